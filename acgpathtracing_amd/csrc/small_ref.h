// small_ref.h — 16-bit node references of the small-scene render kernel (render_small.hip).  Plain functions, host and device.
//
// k_hc_nodes (lbvh_build.hip) writes a child reference as a 32-bit word: an inner node as its byte offset into hcnodes (node index
// * 32), a triangle as ~slot (negative), and the traversal marks "nothing" with kSentinel = 0x7FFFFFFF.  A tree of at most
// kSmallMaxNodes nodes and kSmallMaxTris triangles fits all three into a SIGNED 16-bit entry:
//   inner node   offset / 2            0 .. 32752, a multiple of 16 (the node's offset in 16-byte halves, times 8: << 1 gives the byte offset back)
//   triangle     ~slot, truncated      0x8000 .. 0xFFFF: sign-extended it is ~slot again
//   sentinel     0x7FFF                no multiple of 16, not negative
// The kernel works on the sign-extended entry throughout (small_ref_local): the staged copy of the nodes holds its child words in
// that form, a push stores the low half (ds_write_b16), a pop reads it back sign-extended (ds_read_i16), a triangle is ~node as
// before and an inner node's LDS address is node << 1 — no instruction more than with 32-bit entries.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace ptd {

constexpr int kSmallSentinel = 0x7FFF;               // the sentinel in the kernel's local form
constexpr int kSmallWideSentinel = 0x7FFFFFFF;       // pt_device.h kSentinel (not included here: this header is host code too)
constexpr uint32_t kSmallMaxNodes = 2048u;           // (2048 - 1) * 16 = 32752 < 0x7FFF
constexpr uint32_t kSmallMaxTris = 32768u;           // ~32767 = -32768

__host__ __device__ inline uint16_t small_ref_encode(int ref)
{
    if (ref == kSmallWideSentinel) return (uint16_t)kSmallSentinel;
    return ref < 0 ? (uint16_t)(uint32_t)ref : (uint16_t)((uint32_t)ref >> 1);
}
__host__ __device__ inline int small_ref_decode(uint16_t e)
{
    if (e == (uint16_t)kSmallSentinel) return kSmallWideSentinel;
    return (e & 0x8000u) ? (int)(int16_t)e : (int)((uint32_t)e << 1);
}
// the form the kernel holds in registers and in its copy of the nodes: the entry, sign-extended
__host__ __device__ inline int small_ref_local(int ref) { return (int)(int16_t)small_ref_encode(ref); }

}  // namespace ptd
