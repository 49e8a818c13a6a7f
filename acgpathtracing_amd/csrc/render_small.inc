// render_small.inc — the body of k_render_small (render_small.hip): render_pw.inc at NODE_FMT 14, INNER 6, LEAVES 2, SHADE_K 40,
// LEAF_K 16, light mode 0, no environment map, the reference material model — every other format and every experiment branch
// taken out.  Everything that is under the bit-exact contract is k_render_pw<40,16,11,256,5,false,0,6,2,false,0,0,MATH>'s, operation
// for operation: ray setup, tri_test_lazy, the (t, prim) tie rule, shading, accumulation.  The box test is not under that contract
// and is not variant 7's: slab_hcf / slab_hcf_f32 (small_slab.h) form near and far with one fma each where slab_hc rounds the half
// extent's product first.  A box test only decides which leaves a ray reaches; a hit is decided by tri_test_lazy alone, the closest
// by (t, prim) whatever the order the leaves come in, a shadow ray by any hit, and the counters count rays and paths, not visits.
// So any conservative box test leaves image bits and counters where they are: same image bits, same counters as variant 7, while
// the order in which two children with nearly equal entry distances are walked may differ from variant 7's.  What else differs is
// where things live:
//   * the fp16 nodes are read from a copy in LDS that the workgroup stages once (ds_read_b128), child words rewritten to the
//     16-bit local form of small_ref.h; the texture path sees the triangle records only;
//   * stack entries are 16 bits, entry-major, lane-minor, two lanes to a dword (ds_write_b16 / ds_read_i16);
//   * the wave's number in the grid (fold-slot scratch) starts at B.wave0, so that two launches can share one RenderArgs.
// LDS of a workgroup, in this order: lane stacks (waves x stack_entries x 128 B), nodes (n_lds_nodes x 32 B), LCG table (256 B),
// fold books (waves x kBookDwords x 4 B) — small_lds_bytes() in render_small.hip.
// NODES (render_small.h) says where the nodes are.  kSmallNodesHalfLds is the above.  kSmallNodesFloatLds: the copy holds every fp16
// number as the float it converts to (small_stage_f32: n_lds_nodes x 64 B, a node at node << 2), a visit is four ds_read_b128 and
// two slab_hcf_f32: eighteen full-rate v_fma_f32, the bits of slab_hcf's eighteen v_fma_mix_f32.  kSmallNodesHalfGlobal: no copy;
// a visit reads the fp16 node from sc.hcnodes as variant 7 does and halves an inner child's byte offset on the way to the stack.
// The loop shape can be set from the command line of a scratch build (-DSMALL_INNER=.. -DSMALL_LEAF_K=.. -DSMALL_SHADE_K=..); the
// defaults are what profiles/small_fma_ab.txt measured best.
#ifndef SMALL_INNER
#define SMALL_INNER 6
#endif
#ifndef SMALL_LEAF_K
#define SMALL_LEAF_K 16
#endif
#ifndef SMALL_SHADE_K
#define SMALL_SHADE_K 40
#endif
template <int THREADS, int MATH, int NODES>
__global__ void __launch_bounds__(THREADS, 5)
k_render_small(const SmallArgsBox B)
{
    constexpr int SHADE_K = SMALL_SHADE_K, LEAF_K = SMALL_LEAF_K, INNER = SMALL_INNER, LEAVES = 2;
    constexpr int FM = MATH ? 2 : 0;                  // arithmetic level of the shade phase
    constexpr uint32_t WAVES = THREADS / 64;
    const RenderArgs& A = B.a[0];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t entries = A.stack_entries;
    SmallStack st;
    st.base = (uint16_t*)lds_dyn + wave * (entries * 64u) + lane;
    const DeviceScene sc = A.scene;
    // the nodes behind the stacks, 32 bytes apart as in global memory; a child word becomes its local form on the way in
    const char* const lds_nodes = (const char*)(lds_dyn + WAVES * (entries * 32u));
    if constexpr (NODES == kSmallNodesHalfLds) {
        uint4* dst = (uint4*)(lds_dyn + WAVES * (entries * 32u));
        const uint4* src = (const uint4*)sc.hcnodes;
        for (uint32_t i = threadIdx.x; i < A.n_lds_nodes * 2u; i += THREADS) { uint4 v = src[i]; v.w = (uint32_t)small_ref_local((int)v.w); dst[i] = v; }
    } else if constexpr (NODES == kSmallNodesFloatLds) {
        small_stage_f32((uint4*)(lds_dyn + WAVES * (entries * 32u)), (const uint4*)sc.hcnodes, A.n_lds_nodes * 2u, threadIdx.x, THREADS);
    }
    constexpr uint32_t NODE_DWORDS = NODES == kSmallNodesHalfLds ? 8u : NODES == kSmallNodesFloatLds ? 16u : 0u;      // of the copy in LDS
    uint32_t* const lcg_skip = lds_dyn + WAVES * (entries * 32u) + A.n_lds_nodes * NODE_DWORDS;
    if (threadIdx.x < 32u) { lcg_skip[2u * threadIdx.x] = A.lcg_mul[threadIdx.x]; lcg_skip[2u * threadIdx.x + 1u] = A.lcg_add[threadIdx.x]; }
    const WaveBook book = wave_book(lcg_skip + 64u + wave * kBookDwords, lane);
    __syncthreads();
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int root = sc.n_tris ? 0 : kSmallSentinel;

    QueueState q; q.shard = A.row_interleave == 3u ? 0u : xcc_id(); q.shards_left = 8; q.res_first = 0; q.res_count = 0; q.grant_g0 = 0; q.grp_pxy = 0xFFFFFFFFu; q.grp_seed = 0; q.skipped = 0; q.free_top = kFoldSlots;
    q.reach_bit = A.row_spans != nullptr ? 0x80000000u : 0u;
    float* const scratch = A.wave_scratch + 3u * (size_t)__builtin_amdgcn_readfirstlane((int)(B.wave0 + blockIdx.x * WAVES + wave)) * ((size_t)kFoldSlots << A.chunk_shift);   // wave-uniform: scalar registers
    unsigned long long n_radiance = 0, n_shadow = 0, n_paths = 0, n_pixels = 0, n_culled = 0;

    LanePixel lp; lp.alive = false; lp.new_path = false; lp.pxy = lp.seed = lp.samples_left = lp.tag = 0; lp.result = mk(0.0f);
    uint32_t pseed = 0;
    int depth = 0;
    f3 att = mk(1.0f);
    f3 ro = mk(0.0f), rd = mk(0.0f, 0.0f, 1.0f), rinv = mk(1.0f), gro = mk(0.0f);
    constexpr float rtmin = 0.01f;
    float rtmax = 0.0f, best_t = 0.0f;
    int best_slot = -1; uint32_t best_prim = 0xFFFFFFFFu;
    int node = kSmallSentinel, sp = 0, tos = kSmallSentinel;
    bool shadow_ray = false, shadow_hit = false;
    bool fin_pending = false;                         // ran out of samples inside the camera cull: its run is finished at the next round's start
    // what the closest-hit left for after the shadow ray (see render_pw.inc): four values instead of Pending's ten
    f3 keep_dir = mk(0.0f, 0.0f, 1.0f); float keep_weight = 0.0f; bool keep_done = true, keep_metal = false;

    for (;;) {
        // =========================== shade / regenerate: lanes with no ray in flight ===============
        const auto late = [&]() -> const RenderArgs& { return B.a[opaque_zero()]; };
        bool segment_done = false, started_shadow = false;
        f3 emission = mk(0.0f);
        Pending pd;
        pd.nxt_org = mk(0.0f); pd.nxt_dir = mk(0.0f, 0.0f, 1.0f); pd.radiance = mk(0.0f); pd.weight = 0.0f; pd.done = true;
        if (lp.alive && node == kSmallSentinel) {
            if (shadow_ray) {                                         // shadow ray back
                pd.done = keep_done; pd.weight = keep_weight;
                pd.nxt_dir = keep_dir;
                pd.nxt_org = keep_metal ? ro + keep_dir * 1e-4f : ro;                 // ro is the shadow ray's origin P
                pd.radiance = keep_done ? keep_dir : mk(0.0f);
                if (!shadow_hit) pd.radiance = m_madd<FM>(mk(late().light.emission), pd.weight, pd.radiance);
                shadow_ray = false;
                segment_done = true;
            } else {                                                  // radiance ray back
                bool want_shadow = false;
                f3 P, L; float Ldist;
                if (best_slot >= 0) {
                    want_shadow = shade_hit<FM, false>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, emission, pd, P, L, Ldist);
                } else {                                              // miss
                    pd.radiance = mk(0.0f); pd.weight = 0.0f; pd.done = true;
                }
                lp.result += emission;
                if (want_shadow) {
                    keep_done = pd.done; keep_weight = pd.weight;
                    keep_dir = pd.done ? pd.radiance : pd.nxt_dir;
                    keep_metal = !pd.done && !(pd.nxt_org.x == P.x && pd.nxt_org.y == P.y && pd.nxt_org.z == P.z);
                    ro = P; rd = L;
                    { const RenderArgs& Rs = late(); setup_ray_hc(ro, rd, Rs.scene.hspace, rinv, gro); }
                    rtmax = Ldist - 0.01f; best_t = rtmax; best_slot = -1; best_prim = 0xFFFFFFFFu;
                    node = root; sp = 0; shadow_ray = true; shadow_hit = false; started_shadow = true;
                } else {
                    segment_done = true;
                }
            }
        }
        n_shadow += (unsigned long long)popc(vote(started_shadow));
        bool end = false, finished = false;
        if (segment_done) {
            add_segment<FM>(lp.result, pd.radiance, att);
            const float p = roulette_p<FM>(att);
            const bool rr = rnd(pseed) > p;
            end = pd.done || rr || (uint32_t)depth >= A.maxDepth;
            if (!end) {
                att = roulette_scale<FM>(att, p);
                ro = pd.nxt_org; rd = pd.nxt_dir;
                ++depth;
            } else {
                lp.samples_left--;
                lp.new_path = true;
                if (lp.samples_left == 0u) { lp.alive = false; finished = true; }
            }
        }
        n_paths += (unsigned long long)popc(vote(end));
        finished = finished || fin_pending;
        fin_pending = false;
        n_pixels += (unsigned long long)popc(vote(finished));
        finish_runs(A, q, below, lp, finished, book, scratch);     // before the refill overwrites the lanes' items

        refill_lanes<false, true>(A, late, q, lane, below, lp, lcg_skip, book);
        if (q.skipped != 0u) {      // pixels that cannot reach the scene box: every sample is one radiance segment that misses, one path
            const unsigned long long n = (unsigned long long)q.skipped * A.spp;
            n_radiance += n; n_paths += n; n_culled += n;
            n_pixels += (unsigned long long)q.skipped << A.chunk_shift;
            q.skipped = 0u;
        }

        bool start_radiance = segment_done && !end;
        uint32_t my_culled = 0u;                                      // per lane: the counters are wave-uniform and must not be touched under divergence
        if (lp.alive && lp.new_path) {                                // camera path start
            const RenderArgs& Rc = late();
            const f3 eye = mk(Rc.eye), camU = mk(Rc.U), camV = mk(Rc.V), camW = mk(Rc.W);
            const float fw = (float)(int)Rc.width, fh = (float)(int)Rc.height;
            const f3 elo = Rc.scene.n_tris ? mk(Rc.cull_lo) - eye : mk(1.0f), ehi = Rc.scene.n_tris ? mk(Rc.cull_hi) - eye : mk(-1.0f);
            f3 D;
            for (;;) {
                const float jx = rnd(lp.seed);
                const float jy = rnd(lp.seed);
                D = camera_dir<FM>((float)(lp.pxy & 0xFFFFu), (float)(lp.pxy >> 16), jx, jy, fw, fh, camU, camV, camW);
                if ((lp.tag & (1u << 24)) != 0u || reaches_scene(D, elo, ehi)) break;      // bit 24: every ray of this pixel reaches the box
                my_culled++;
                lp.samples_left--;
                if (lp.samples_left == 0u) { lp.alive = false; fin_pending = true; break; }
            }
            if (lp.alive) {
                rd = m_normalize<FM>(D);
                ro = eye;
                att = mk(1.0f);
                pseed = lp.seed;
                depth = 0;
                lp.new_path = false;
                start_radiance = true;
            }
        }
        if (vote(my_culled != 0u) != 0ull) {                           // wave sum of the per-lane counts, bit plane by bit plane
            unsigned long long sum = 0ull;
            for (uint32_t b = 0; vote((my_culled >> b) != 0u) != 0ull; b++) sum += (unsigned long long)popc(vote(((my_culled >> b) & 1u) != 0u)) << b;
            n_radiance += sum; n_paths += sum; n_culled += sum;
        }
        if (vote(lp.alive) == 0ull) { if (q.shards_left == 0u && q.res_count == 0u && vote(fin_pending) == 0ull) break; else continue; }
        if (start_radiance) {
            { const RenderArgs& Rs = late(); setup_ray_hc(ro, rd, Rs.scene.hspace, rinv, gro); }
            rtmax = 1e16f; best_t = rtmax; best_slot = -1; best_prim = 0xFFFFFFFFu;
            node = root; sp = 0; shadow_ray = false;
        }
        n_radiance += (unsigned long long)popc(vote(start_radiance));

        // =========================== traversal: until SHADE_K lanes are parked =====================
        const unsigned long long alive_mask = vote(lp.alive);          // fixed while the wave traverses
        for (;;) {
            const bool act = node != kSmallSentinel;
            const unsigned long long am = vote(act);
            if (am == 0ull) break;
            if (popc(alive_mask & ~am) >= SHADE_K) break;              // parked lanes: scalar arithmetic on the two masks
#pragma unroll
            for (int visit = 0; visit < INNER; visit++)
            if ((uint32_t)node < (uint32_t)kSmallSentinel) {
                float n0, f0, n1, f1;
                int c0, c1;
                if constexpr (NODES == kSmallNodesFloatLds) {
                    uint4 ca, ha, cb, hb;
                    small_node_f32(lds_nodes + ((uint32_t)node << 2), ca, ha, cb, hb);
                    c0 = (int)ca.w; c1 = (int)cb.w;
                    slab_hcf_f32(ca, ha, rinv, gro, rtmin, n0, f0);
                    slab_hcf_f32(cb, hb, rinv, gro, rtmin, n1, f1);
                } else if constexpr (NODES == kSmallNodesHalfGlobal) {
                    // as variant 7 reads them; min(c >> 1, c) is small_ref_local(c) for every word a node holds: ~slot stays, a byte offset is halved
                    const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)((uint32_t)node << 1));
                    const uint4 qa = np[0], qb = np[1];
                    c0 = min((int)qa.w >> 1, (int)qa.w); c1 = min((int)qb.w >> 1, (int)qb.w);
                    slab_hcf(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_hcf(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                } else {
                    uint4 qa, qb;
                    small_node(lds_nodes + ((uint32_t)node << 1), qa, qb);
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    slab_hcf(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_hcf(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                }
                f0 = fminf(f0, best_t * kTieWiden);
                f1 = fminf(f1, best_t * kTieWiden);
                const bool h0 = n0 <= f0, h1 = n1 <= f1;
                // elements e_1..e_sp, e_sp in `tos`, e_k (k < sp) in LDS slot k
                const bool first0 = n0 <= n1;
                const int near_c = (h0 && (first0 || !h1)) ? c0 : c1;
                const int far_c = first0 ? c1 : c0;
                if (h0 && h1) { st.push(sp, tos); tos = far_c; sp++; }
                if (h0 || h1) {
                    node = near_c;
                } else {
                    node = sp ? tos : kSmallSentinel;
                    sp = sp ? sp - 1 : 0;
                    tos = st.pop(sp);
                }
            }
            const bool at_leaf = node < 0;       // the sentinel is positive
            const unsigned long long lm = vote(at_leaf);
            if (lm != 0ull && (popc(lm) >= LEAF_K || vote(node >= 0 && node != kSmallSentinel) == 0ull)) {
#pragma unroll
                for (int leaf = 0; leaf < LEAVES; leaf++)          // a lane whose next node is a leaf again tests it in the same round
                if (node < 0) {
                    const int slot = ~node;
                    const TriRecord* tp = (const TriRecord*)((const char*)sc.tris + (size_t)((uint32_t)slot * 48u));
                    const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
                    float t;
                    const bool ok = tri_test_lazy(ro, rd, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), rtmin, rtmax, t);
                    const uint32_t prim = __float_as_uint(r2.y);
                    bool stop = false;
                    if (ok) {
                        if (shadow_ray) { shadow_hit = true; stop = true; }
                        else if (t < best_t || (t == best_t && prim < best_prim)) { best_t = t; best_slot = slot; best_prim = prim; }
                    }
                    node = (stop || sp == 0) ? kSmallSentinel : tos;
                    sp = sp ? sp - 1 : 0;
                    tos = st.pop(sp);
                }
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&A.counters[0], n_radiance);
        atomicAdd(&A.counters[1], n_shadow);
        atomicAdd(&A.counters[2], n_paths);
        atomicAdd(&A.counters[3], n_pixels);
        if (n_culled) atomicAdd(&A.counters[kCulledCounter], n_culled);
    }
}
