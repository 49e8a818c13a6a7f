// bvh_walk.h — the one stack walk of the query kernels over the scene's two-child BVH.  nearest.hip,
// nearest_k.hip, segment.hip, tridist.hip, multihit.hip, overlap.hip, oriented.hip, tritri.hip, lists.hip and poses.hip walk through
// it with policies of their own, and the casts (sweep.hip, capsule.hip, boxcast.hip, tricast.hip) with the one policy of cast_walk.h;
// the render kernels (pt_device.h, traverse_hc.h) and winding.hip, which walks its own node record, keep their loops.
//
// What the walk guarantees, whatever the policy:
//   * One query per lane.  An inactive lane (a lane past n, a query that is a miss before any traversal) and every lane of an empty
//     scene fall straight through; they stay in the wave.
//   * A visit of an inner node decodes its two children — the fp16 centre / half-extent node of sc.hcnodes (FMT 11) or the fp32
//     BvhNode of sc.nodes (FMT 0) —, asks the policy which are admitted and which of two admitted ones goes first, enters that one
//     and pushes the other.  So a visit pushes at most one reference and descends one level: the references on the stack belong to
//     siblings of nodes on the current root-to-node path, at most one per level, and the depth the ray walks need (size_stack,
//     capi.hip: max_depth + 1) holds here too.
//   * A popped reference is entered without a second look at its own box — its children are tested against the policy's state of
//     that moment, a popped leaf is tested —, so a stack entry is one word.
//   * The boxes only prune.  What a query finds is decided by the policy's leaf test alone, whatever order the walk reaches the
//     triangles in; every triangle sits in one leaf, so each is tested at most once.  (The one node of a single-triangle scene names
//     its triangle in both children, the second under an empty box: a policy must not admit an empty child.)
//
// The policy is a small struct in the query's own file that holds all of the lane's mutable state (best candidate, threshold or
// cut, list, count):
//   void children_hc(const uint4& qa, const uint4& qb, const HSpace& hs, bool& h0, bool& h1, bool& first0)
//        qa, qb: the two children's packed centre / half-extent words (x, y, z; .w is the reference and the walk's business)
//   void children_f32(const float4& a, const float4& b, const float4& c, bool& h0, bool& h1, bool& first0)
//        the raw node words: child 0 lo (a.x a.y a.z) hi (a.w b.x b.y), child 1 lo (b.z b.w c.x) hi (c.y c.z c.w)
//        h0, h1: the child is admitted; first0: of two admitted children, child 0 is entered and child 1 pushed (a walk that keeps
//        the tree's order sets true)
//   bool leaf(int slot, const float4& r0, const float4& r1, const float4& r2)
//        the TriRecord of sc.tris[slot]: v0 (r0.x r0.y r0.z), e1 (r0.w r1.x r1.y), e2 (r1.z r1.w r2.x), the triangle index r2.y.
//        true: the lane is finished (the "any" forms)
// VISITS counts the inner nodes visited (visits.x) and the triangles tested (visits.y): the test hooks' instantiations.
#pragma once
#include "query_launch.h"

namespace ptd {

template <int FMT, bool VISITS, class P>
__device__ __forceinline__ void bvh_walk(const DeviceScene& sc, const LaneStack& st, bool active, P& policy, uint2& visits)
{
    int sp = 0;
    int node = (active && sc.n_tris != 0u) ? 0 : kSentinel;
    while (node != kSentinel) {
        if (node >= 0) {
            bool h0, h1, first0;
            int c0, c1;
            if (FMT == 11) {
                // child references of inner nodes are byte offsets into hcnodes; a leaf is ~slot
                const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                const uint4 qa = np[0], qb = np[1];
                policy.children_hc(qa, qb, sc.hspace, h0, h1, first0);
                c0 = (int)qa.w; c1 = (int)qb.w;
            } else {
                const BvhNode* np = sc.nodes + node;
                const float4 a = np->a, b = np->b, c = np->c;
                const int4 ch = np->d;
                policy.children_f32(a, b, c, h0, h1, first0);
                c0 = ch.x; c1 = ch.y;
            }
            if (VISITS) visits.x++;
            if (h0 && h1) {
                st.push(sp, first0 ? c1 : c0);
                sp++;
                node = first0 ? c0 : c1;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else {
                if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
            }
        } else {
            const int slot = ~node;
            const TriRecord* tp = sc.tris + slot;
            const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
            if (VISITS) visits.y++;
            if (policy.leaf(slot, r0, r1, r2)) { node = kSentinel; continue; }
            if (sp == 0) node = kSentinel; else { sp--; node = st.pop(sp); }
        }
    }
}

// The admission of the walks that are ordered by a lower bound of the squared distance to each child box (nearest, nearest_k,
// within_any, segments, triangle distance): a child is entered iff its bound is at most thr — false for an empty child's NaN —, and
// of two such children the nearer goes first.
__device__ __forceinline__ void admit_by_bound(float b0, float b1, float thr, bool& h0, bool& h1, bool& first0)
{
    h0 = b0 <= thr; h1 = b1 <= thr;
    first0 = b0 <= b1;
}

// The admission of the walks that clip a line against each child box (sweep, multi-hit): a child is entered iff its interval
// [n, f] is not empty — false for a NaN —, and of two such children the one entered earlier goes first.
__device__ __forceinline__ void admit_by_interval(float n0, float f0, float n1, float f1, bool& h0, bool& h1, bool& first0)
{
    h0 = n0 <= f0; h1 = n1 <= f1;
    first0 = n0 <= n1;
}

}  // namespace ptd
