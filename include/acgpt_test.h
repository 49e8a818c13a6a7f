/*
 * acgpt_test.h — test hooks and diagnostics of libacgpt_hip.so.
 *
 * NOT part of the drop-in boundary (include/acgpt.h): nothing here stands in for a function of the reference's
 * PathTracerMain.cpp.  The parity tests and the tools under tools/ use these to hold the device functions against golden
 * vectors and to look inside the scheduler; a binding of the render path never needs them.
 */
#ifndef ACGPT_TEST_H
#define ACGPT_TEST_H

#include "acgpt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: pure-traversal throughput.  Streams n HOST rays (same 8-float records; tmax < 0 marks an
 * any-hit ray of length |tmax|) through a persistent kernel that contains nothing but the BVH loop, `repeats`
 * times, and reports the fastest kernel time.  node_format 0: two-child fp32 tree; 1: four-wide 8-bit tree;
 * 2: two-child tree with the slab test as one fma per plane (the fp32 render kernels' form); 3: fp16 {lo, hi} nodes (rounds 2-3's default);
 * 4: fp16 {centre, half extent} nodes with a scale per axis — the array and the box test the default render kernels use.
 * Results: closest rays as pt_trace_closest; any-hit rays give t_out = prim_out = 1 when occluded, 0
 * otherwise.  counters_out (may be NULL): 5 values of the last repeat — loop iterations summed over waves,
 * node visits summed over lanes, triangle tests summed over lanes, iterations with a node visit, iterations
 * with a triangle round.  Not used by the render path.                                                   */
int pt_bench_traversal(pt_ctx* ctx, const float* rays, size_t n, int repeats, int node_format, float* t_out, uint32_t* prim_out, float* ms_out,
                       uint64_t* counters_out);
/* Test hook: evaluates the device functions the render kernel is built from on HOST inputs (n elements), so that
 * the GPU implementations can be held against golden vectors of the reference's own code directly.
 *   op 0  tea<4> (cuda/random.h:31-46)            in uint32[n][2]                 out uint32[n]
 *   op 1  lcg / rnd stream (cuda/random.h:49-67)  in {seed, count}, n = 1         out uint32 states[count], float values[count]
 *   op 2  make_color (cuda/helpers.h:35-62)       in float[n][3]                  out uchar4[n]
 *   op 3..8 normalize, reflect, faceforward, lerp, cross, a / s (sutil/vec_math.h)  in float[n][10] = a, b, c, s   out float[n][3]
 *   op 9  refract (cuda/helpers.h:107-137)        in float[n][7] = i, n, ior      out float[n][4] = r, ok (uint32)
 *   op 10 StaticWorkDistribution::getSamplePixel (sutil/WorkDistribution.h:59-81)  in int32[n][4] = world, width, rank, sample   out int32[n][2]
 *   op 11 sinf(x), cosf(x) and the pair sincosf(x) gives (the samplers use the latter)   in float[n]   out float[n][4]
 * the OptiX-free helpers of pathTracerPrograms.cu, golden vectors from the reference's own text (oracle/_ref):
 *   op 12 OrthonormalBasis(n).inverse_transform(p) (:54-85)        in float[n][6] = n, p            out float[n][3]
 *   op 13 safeDivide(float3, float) (:265-284)                      in float[n][4] = a, b            out float[n][3]
 *   op 14 cosine_sample_hemisphere (:341-353)                       in float[n][2] = eta1, eta2      out float[n][3]
 *   op 15 uniform_sample_hemisphere (:368-380)                      in float[n][2] = u1, u2          out float[n][3]
 *   op 16 sampleGGX (:455-476)                                      in float[n][6] = u1, u2, roughness, N   out float[n][3]
 *   op 17 fresnelSchlickConductor (:494-510)                        in float[n][7] = cosTheta, eta, k       out float[n][3]
 *   op 18 FrDielectric (:534-559)                                   in float[n][3] = cosThetaI, etaI, etaT  out float[n][1]
 * and the default kernel's own ray / box test (no reference counterpart: OptiX traverses there), end to end:
 *   op 19 fp16 slab test: box -> outward fp16 planes, ray -> per-axis multiplier / addend with the rotate flags in the
 *         multiplier's low bits, entry / exit distance          in float[n][17] = ray o, d, box lo, hi, scene centre, inv_scale
 *         (the builder's: scene half extent / 1023; any positive value), tmax    out uint32[n][3] = accepted, entry t (float bits), exit t (float bits).  Must accept every
 *         ray that meets the box shrunk by the builder's pad (tests/test_gpu_golden.py).
 * the arithmetic of PT_MATH_FAST (pt_set_math_mode; no reference vectors exist for it: nvcc's approximate instructions are not
 * reproducible here — the ops are held against their IEEE twins by error bounds):
 *   op 30 primitives      in float[n][2] = a, b     out float[n][4] = a * rcp(b), sqrt(|a|), x and y of normalize((a, b, 1))
 *   op 31 sin / cos of 2 pi u                       in float[n]     out float[n][4] = v_sin_f32(u), v_cos_f32(u), sinf(2 pi u), cosf(2 pi u)
 *   op 32..38 = ops 12..18 at that level, same records (op 33: the roulette's throughput scaling, one reciprocal for the three quotients)
 *   op 40 = op 19 (same records, same outputs) through the fp16 centre / half-extent form of the nodes (NODE_FMT 11: pack_centre_half, slab_hc)
 *   op 41 = op 40 with a scale per axis, as the builder uses it: in = ray o xyz, d xyz, box lo xyz, hi xyz, scene centre xyz, inv_scale xyz, tmax (19 floats)
 *   op 42 = op 41 (same records, same outputs) through the small-scene kernel's box test on the packed fp16 words (csrc/small_slab.h slab_hcf:
 *         near and far by one fma each); op 43 = op 42 on the operands converted to fp32 first, as the kernel stages them in LDS (slab_hcf_f32):
 *         the same bits as op 42 in all three words
 *   op 39 shared-plane slab test (NODE_FMT 10, pt_device.h SSpace): in float[n][20] = ray o xyz, d xyz, box lo xyz, hi xyz, root planes L xyz, H xyz,
 *         inv_scale, tmax; the box as child 0 and as child 1 of a node whose other child is the root box.  out uint[n][3] = accepted as child 0,
 *         accepted as child 1, root accepted | sibling (the root box) accepted << 1 | << 2 */
int pt_selftest(pt_ctx* ctx, int op, const void* in, size_t n, void* out);
/* Diagnostic: after a launch of a "+ scheduler stats" kernel variant, three 100 MHz stamps per wave (start,
 * first time it found the work queue empty, end; 0 = wave did not run), HOST output of 3 * max_waves values. */
int pt_debug_wave_times(pt_ctx* ctx, uint64_t* out, size_t max_waves);
/* ... and, per work-queue shard (8), the stamp of the first grant past each 1/256 of the shard: HOST output of
 * 8 * 256 values (0 = never reached by a stamped grant), followed by ONE value: the time all waves together spent
 * in the shade / regenerate phase, in 10 ns units and its split into queue refill / finished runs / camera-path start (2056 values in all: 2048 + 1 + 3, rest unused). */
int pt_debug_queue_progress(pt_ctx* ctx, uint64_t* out);
/* Order of the work queue over its eight shards (one per XCD).  0: each shard is a contiguous eighth of the 8x4-tile order
 * (round 2); 1 (default): tile-strip rows are dealt round robin over the shards (what sutil/WorkDistribution.h:60-81 does
 * across GPUs); 2: single tiles round robin; 3: one queue in image order.  Same image bits and counters in every mode. */
int pt_debug_queue_order(pt_ctx* ctx, int mode);
/* Pixel classes on (default) / off.  On: per image row, the host hands the kernel the columns outside which no ray of a pixel can
 * reach the scene's bounding box (those pixels' samples are booked as misses without being started) and the columns inside
 * which every ray does (their path starts skip the cull test).  Same image bits and the same ray / path counters either way;
 * pt_stats.culled_rays differs (it counts what was settled without a traversal). */
int pt_debug_pixel_classes(pt_ctx* ctx, int on);
/* The host computation behind them, callable without a context or a GPU: for the camera and image size of `params` and the box
 * [box_lo, box_hi], out[2 * y] = outer columns lo | hi << 16 and out[2 * y + 1] = inner columns lo | hi << 16 of image row y
 * (2 * height words).  0 = computed, 1 = no classes for this view (box not entirely in front of the eye, degenerate frame). */
int pt_debug_row_spans(const pt_params* params, const float* box_lo, const float* box_hi, uint32_t* out);
/* Diagnostic, one value of the last launch: a windowed-stack kernel's moves of stack entries between the LDS window and global
 * memory (wave-level events; 0 for the kernels that keep the whole stack in LDS). */
int pt_debug_window_moves(pt_ctx* ctx, uint64_t* out);
/* The small-scene path (csrc/render_small.hip): where the library chose the default kernel itself, light mode 0, no map, the reference
 * material model, a context of its own (no pt_create_multi group), and the scene's fp16 nodes fit a CU's LDS twice beside the stacks of 20 waves, a launch runs one 1024-thread
 * and one 256-thread workgroup per CU that read the nodes from LDS.  mode 0: automatic (default); 1: off, the variant table's kernel
 * as before; 2 / 3: the 1024- / 256-thread grid alone.  Same image bits and counters in every mode; pt_stats.variant stays the variant the path stands in for. */
int pt_debug_small_kernel(pt_ctx* ctx, int mode);
/* ... and what the context's last launch ran: 0 the variant table's kernel, 1 both grids, 2 / 3 the 1024- / 256-thread grid alone. */
int pt_debug_small_kernel_path(pt_ctx* ctx);
/* The path's 16-bit node references (csrc/small_ref.h), no context, no GPU: for each of n 32-bit references as the tree holds them
 * (byte offset of an inner node, ~slot of a triangle, 0x7FFFFFFF for "nothing") the 16-bit entry, what it decodes to, and the
 * sign-extended entry the kernel works on.  HOST arrays of n. */
int pt_debug_small_ref(const int32_t* refs, size_t n, uint16_t* encoded, int32_t* decoded, int32_t* local);
/* ... and its LDS budget: out[0], out[1] = dynamic LDS bytes of the 1024- and the 256-thread workgroup for a tree of n_nodes nodes and
 * stack_entries entries per lane, out[2] = 1 when such a scene with n_tris triangles is eligible on a CU with cu_lds_bytes of LDS (one
 * workgroup of each kind fits, a second 256-thread one beside them does not, references fit 16 bits), out[3], out[4] = the node and
 * triangle limits of the references. */
int pt_debug_small_budget(uint32_t n_nodes, uint32_t n_tris, uint32_t stack_entries, uint64_t cu_lds_bytes, uint64_t* out);
/* Inside the path a launch has one of two shapes.  2: the 1024-thread workgroup holds the nodes as fp32 (64 bytes a node: every fp16
 * number converted once, at staging, instead of at every visit) and the 256-thread workgroup holds no copy and reads the fp16 nodes
 * from global memory; taken where that budget fits the CU.  1: both workgroups hold the fp16 nodes, as described above; the fallback.
 * Returns the shape of the context's last launch (0: it did not take the path; -1: bad argument), and sets which to take from now on:
 * force 0 automatic (default), 1 the fp16 shape always, -1 no change.  Same image bits and counters either way. */
int pt_debug_small_shape(pt_ctx* ctx, int force);
/* ... the budget of shape 2, no context, no GPU: out[0] = LDS bytes of the 1024-thread workgroup (stacks, books, LCG table, n_nodes x
 * 64), out[1] = of the 256-thread workgroup (stacks, books, LCG table), out[2] = what the 256-thread launch asks for: out[1] padded
 * to just over half of what the 1024-thread workgroup leaves free, so that out[0] + 2 x out[2] > cu_lds_bytes and a CU never holds
 * two of them, out[3] = 1 when out[0] and out[1], each counted up to a whole KB, fit cu_lds_bytes together. */
int pt_debug_small_float_budget(uint32_t n_nodes, uint32_t stack_entries, uint64_t cu_lds_bytes, uint64_t* out);
/* ... and the fp32 nodes as the 1024-thread workgroup stages them, by the kernel's own staging function run over the scene's fp16
 * nodes: 64 bytes a node into a HOST buffer; per child {(float) centre x, y, z, child reference in the 16-bit local form} and
 * {(float) half extent x, y, z, 0}. */
int pt_debug_small_staged(pt_ctx* ctx, void* out, size_t capacity_bytes);
#ifdef ACGPT_EXPERIMENTS
/* Experiments library only: walk a renumbered copy of the fp16 nodes (0: the build's order; 1: the two children of a node in one 64-byte
 * line; 2: depth first).  Same bits; an A/B of the memory system on large scenes (profiles/r04_ab_node_order.txt). */
int pt_debug_node_order(pt_ctx* ctx, int mode);
/* Experiments library only (libacgpt_hip_exp.so, -DACGPT_EXPERIMENTS; never the product): 17 values after a launch of a wavefront
 * kernel variant (render_wavefront.hip), summed over the waves of the grid, times in 10 ns ticks: trace waves {total, idle},
 * shade waves {total, idle, deal time / rounds / records, hit-shading time / rounds / records, accounting time / rounds /
 * records}, trace waves {exchange time / exchanges / records taken in, loop trips}. */
int pt_debug_wf(pt_ctx* ctx, uint64_t* out);
#endif
/* The environment map's device functions (csrc/pt_environment.h, what the render kernels call) in the context's math mode, for n
 * queries, HOST arrays.  op 0: unit direction {x, y, z} -> {r, g, b, texel index (-1 without a map)}; op 1: direction -> solid-angle
 * pdf of the map's sampling; op 2: {u1, u2} in [0, 1)^2 -> {x, y, z, pdf} of the sampled direction (pdf 0: nothing to sample). */
int pt_debug_environment(pt_ctx* ctx, int op, const float* in, size_t n, float* out);
/* The tables of the context's map as the device holds them right now (csrc/environment.hip builds them), copied to HOST arrays:
 * texels float[h][w][4] = {r, g, b with the scale applied, the sampling weight the kernel wrote}, marginal float[h], conditional
 * float[h][w], info2 = {total weight, pdf_scale}.  A NULL pointer skips that array.  Device-to-host copies after a stream
 * synchronisation only: no kernel, nothing is built or released.  dims2 (may be NULL) = {width, height}, {0, 0} without a map.
 * Returns 1 when a map is set and the arrays were filled, 0 when none is (the arrays are left alone), -1 for a null context or a
 * failed copy (the text is in pt_last_error).  A pt_create_multi context reads rank 0.  tests/test_gpu_env_wide.py. */
int pt_debug_environment_tables(pt_ctx* ctx, float* texels, float* marginal, float* conditional, float* info2, uint32_t* dims2);
/* The microfacet BSDF of pt_set_material_model(1) (csrc/pt_microfacet.h) in the context's math mode, for n items of 9 floats,
 * normal (0, 0, 1) face-forwarded to wo (wo.z < 0: leaving a dielectric's inside):
 *   op 0: {wo[3], alpha, ior, bsdf, u1, u2, u3} -> {wi[3], weight[3], pdf, lobe (0 ended, 1 reflection, 2 transmission)}
 *   op 1: {wo[3], wi[3], alpha, ior, bsdf} -> {f[3], pdf}.  HOST arrays. */
int pt_debug_microfacet(pt_ctx* ctx, int op, const float* in, size_t n, float* out);
/* pt_query_nearest (same arguments, same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner
 * nodes query i visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  tools/nearest_timing.py. */
int pt_debug_nearest_visits(pt_ctx* ctx, const float* points, size_t n, pt_nearest* out, uint32_t* visits);
/* pt_query_overlap's counting walk (max_prims = 0: the same boxes, the same counts, the same refusals) from a kernel instantiation
 * that also counts its work: visits[2 i] = inner nodes box i visited, visits[2 i + 1] = triangles it tested.  counts: DEVICE, n words;
 * visits: DEVICE, 8-byte aligned, 2 n words; neither may be null.  tools/overlap_timing.py. */
int pt_debug_overlap_visits(pt_ctx* ctx, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits);
/* Its twin for pt_query_overlap_oriented's 64-byte records: the same counts, the same refusals.  tools/oriented_timing.py. */
int pt_debug_overlap_oriented_visits(pt_ctx* ctx, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits);
/* The same counting walk with the nine axes cross(world axis, box axis) added to its admission: the other arm of the six-against-
 * fifteen-axis measurement.  The same counts; no call of include/acgpt.h walks this way. */
int pt_debug_overlap_oriented_visits_cross(pt_ctx* ctx, const float* boxes, size_t n, uint32_t* counts, uint32_t* visits);
/* pt_query_sweep (same arguments, same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner nodes
 * sweep i visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  tools/sweep_timing.py. */
int pt_debug_sweep_visits(pt_ctx* ctx, const float* sweeps, size_t n, pt_sweep_hit* hits, uint32_t* visits);
/* pt_query_capsule_cast (same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner nodes cast i
 * visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  mode: 0 the product's walk, 1 the walk
 * without the plane axis (the box's separation from the plane of the swept axis), which changes the counts and never the records;
 * anything else is refused.  tools/capsule_timing.py. */
int pt_debug_capsule_cast_visits(pt_ctx* ctx, const float* casts, size_t n, pt_capsule_cast_hit* hits, uint32_t* visits, uint32_t mode);
/* pt_query_box_cast (same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner nodes cast i
 * visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  mode: 0 the walk with the six extra axes
 * (the box's own axes against the swept interval, and cross(box axis, d)), 1 the walk on the inflated slab alone, which changes the
 * counts and never the records; anything else is refused.  tools/boxcast_timing.py. */
int pt_debug_box_cast_visits(pt_ctx* ctx, const float* casts, size_t n, pt_box_cast_hit* hits, uint32_t* visits, uint32_t mode);
/* pt_query_triangles' counting walk (max_prims = 0: the same triangles, the same counts, the same refusals) from a kernel
 * instantiation that also counts its work: visits[2 i] = inner nodes query i visited, visits[2 i + 1] = triangles it tested.  counts:
 * DEVICE, n words; visits: DEVICE, 8-byte aligned, 2 n words; neither may be null.  tools/triangles_timing.py. */
int pt_debug_triangles_visits(pt_ctx* ctx, const float* tris, size_t n, uint32_t* counts, uint32_t* visits);
/* pt_query_segments (same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner nodes segment i
 * visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  flags: 0, or 1 to switch off the walk's
 * second box bound (the three axes perpendicular to the segment), which changes the counts and never the records; anything else is
 * refused.  tools/segments_timing.py. */
int pt_debug_segments_visits(pt_ctx* ctx, const float* segments, size_t n, pt_segment_hit* out, uint32_t* visits, uint32_t flags);
/* pt_query_triangle_distance (same records, same refusals) from a kernel instantiation that also counts: visits[2 i] = inner nodes
 * query i visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.  flags: 0, or 1 to switch off the
 * walk's second box bound (the separation along the query triangle's normal), which changes the counts and never the records;
 * anything else is refused.  tools/tridist_timing.py. */
int pt_debug_triangle_distance_visits(pt_ctx* ctx, const float* tris, size_t n, pt_triangle_distance_hit* out, uint32_t* visits, uint32_t flags);
/* pt_query_poses_distance (out given; hit and first must be null) or pt_query_poses_any (out null; hit given, first optional), with
 * the same answers and the same refusals, from launches that take flags: bit 0 switches the early look at the pose's word and the
 * shrinking radius off, so that every lane walks as the per-triangle kernels do; bit 1 deals the lanes pose-major (consecutive lanes
 * on consecutive triangles of one pose) instead of triangle-major (all poses' triangle 0 first, the product's order).  Neither changes an output bit.  max_radius is read with out only.  Anything above 3 is
 * refused.  tools/poses_timing.py. */
int pt_debug_query_poses(pt_ctx* ctx, const float* poses, size_t P, float max_radius, uint8_t* hit, uint32_t* first, pt_pose_distance_hit* out, uint32_t flags);
/* pt_query_triangle_cast (same arguments, same records, same refusals) from a kernel instantiation that also counts: visits[2 i] =
 * inner nodes cast i visited, visits[2 i + 1] = triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words.
 * tools/tricast_timing.py. */
int pt_debug_triangle_cast_visits(pt_ctx* ctx, const float* casts, size_t n, pt_triangle_cast_hit* hits, uint32_t* visits);
/* pt_query_poses_cast (same answers, same refusals) from launches that take pt_debug_query_poses' flags: bit 0 switches the early look
 * at the pose's word and the shrinking tmax off, bit 1 deals the lanes pose-major.  Neither changes an output bit.  Anything above 3
 * is refused. */
int pt_debug_query_poses_cast(pt_ctx* ctx, const float* poses, const float* motions, size_t P, pt_triangle_cast_hit* out, uint32_t flags);
/* pt_query_nearest_k (hit null: same records, same counts, same refusals) or pt_query_within_any (hit given; max_k must be 0 and
 * out and counts null) from kernel instantiations that also count: visits[2 i] = inner nodes point i visited, visits[2 i + 1] =
 * triangles it tested.  visits: DEVICE, 8-byte aligned, 2 n words, never null.  tools/nearest_k_timing.py. */
int pt_debug_nearest_k_visits(pt_ctx* ctx, const float* points, size_t n, uint32_t max_k, pt_nearest* out, uint32_t* counts, uint8_t* hit, uint32_t* visits);
/* pt_query_winding (same bits, same refusals) from a kernel instantiation that also counts: visits[2 i] = dipoles point i took,
 * visits[2 i + 1] = triangles it evaluated.  visits: DEVICE, 8-byte aligned, 2 n words, never null.  tools/winding_timing.py. */
int pt_debug_winding_visits(pt_ctx* ctx, const float* points, size_t n, float beta, float* out, uint32_t* visits);
/* pt_query_winding's moments to the HOST as the device holds them: n_nodes records of 32 bytes {p[3], r2, N[3], A} in the scene's
 * node numbering (pt_debug_read_tree's).  Never builds them: refused while they are not built (pt_get_winding_info), and on a
 * capacity below their size, a null context or a null out. */
int pt_debug_read_winding(pt_ctx* ctx, void* out, size_t capacity_bytes);
/* Which parts of pt_query_overlap_lists / pt_query_triangles_lists run on this context from now on, for timing them apart
 * (tools/lists_timing.py): 1 the fill alone (long slices stay in walk order), 2 the sort alone (of what prims holds), 3 both (the
 * default, the product), plus 4 for a fill that keeps no sorted register list, so that every slice of two words or more goes through
 * the sort.  3 and 7 give the same lists.  Anything else is refused. */
int pt_debug_list_phases(pt_ctx* ctx, uint32_t phases);
/* Sorted (morton, triangle) pairs of the last build, HOST outputs of n_tris. */
int pt_read_morton(pt_ctx* ctx, uint32_t* codes_sorted, uint32_t* prims_sorted);
/* What the scene's tree is made of, as the device holds it right now (tests/tree_ref.py validates it node by node).  Not part of the
 * ABI (pt_abi_version stays as it is): a plain struct of this header. */
typedef struct pt_tree_info {
    uint32_t n_tris, n_nodes, max_depth;
    int32_t  mode;                  /* the build mode the tree was made with (0 Karras, 1 PLOC, 2 PLOC + reinsertion) */
    float    pad_abs;               /* absolute pad of the triangle boxes */
    float    hspace[8];             /* cx, cy, cz, inv_scale, isx, isy, isz, pad_ : the space of the fp16 planes */
    float    scene_lo[3], scene_hi[3];
    uint32_t n_wrecs, n_wnodes, wide_depth;
    uint32_t held;                  /* bit (what - 1) set: array `what` below is on the device */
} pt_tree_info;
/* Copies one array of the scene's tree to the HOST, as it is held right now: what = 0 info only (out may be NULL); 1 fp32 nodes
 * (64 B each, n_nodes); 2 fp16 {lo, hi} nodes (32 B); 3 fp16 {centre, half extent} nodes (32 B; inner child references are byte
 * offsets); 4 four-wide records (48 B, n_wrecs); 5 triangle records (48 B, n_tris, Morton order); 6 shade records (16 B, n_tris).
 * Never allocates, never brings an array into existence and leaves pt_get_bvh_info().device_bytes as it is: an array that is not held,
 * a capacity below the array's size, a missing scene or a null argument is refused.  info may be NULL (what != 0).  A
 * pt_create_multi context reads rank 0. */
int pt_debug_read_tree(pt_ctx* ctx, int what, void* out, size_t capacity_bytes, pt_tree_info* info);
/* What the last build recorded about itself (tests/build_ref.py holds each figure to a sequential reference).  Not part of the ABI
 * (pt_abi_version stays as it is). */
typedef struct pt_build_stats {
    float    opt_area_before, opt_area_after;   /* build mode 2: sum of the inner nodes' surface areas before / after the optimisation; 0 where none ran */
    float    opt_ms;                            /* host time of the optimisation */
    uint32_t opt_passes;                        /* passes of the host insertion / rounds of the device reinsertion that ran */
    uint32_t build_iterations;                  /* PLOC merge rounds (modes 1 and 2) */
    int32_t  mode;                              /* the build mode the tree was made with */
} pt_build_stats;
/* Fills *out from the context alone: no device call, nothing built or released.  Refused, with *out left as it is: a null context, a
 * null out, no scene. */
int pt_debug_build_stats(pt_ctx* ctx, pt_build_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* ACGPT_TEST_H */
