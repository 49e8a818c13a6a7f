// render_pw.inc — the body of the persistent path-trace kernel (render_megakernel.hip), included there four times:
//   RENDER_PW_ENV 0: k_render_pw(const RenderArgsBox), the kernels without an environment map;
//   RENDER_PW_ENV 1: k_render_env(const RenderArgsEnvBox), the same kernel with the map of pt_set_environment (pt_environment.h) on
//                    miss: a radiance ray that leaves the scene and a camera ray the cull settles see the map, the pixel class
//                    "outside" is not applied (its pixels see the map too); with LIGHTS the map is also a light (shade_hit_lights).
//   RENDER_PW_GGX 1: k_render_ggx(const RenderArgsGgxBox) and, with RENDER_PW_ENV 1, k_render_ggx_env(const RenderArgsGgxEnvBox):
//                    the LIGHTS kernels with the microfacet material model (pt_set_material_model; shade_hit_micro, pt_microfacet.h),
//                    the per-material alpha behind RenderArgs (and the map).
// Several kernels from one text rather than one kernel template with a flag, so that k_render_pw is compiled exactly as it was before
// the map existed (an inlined body behind a wrapper, or a larger RenderArgs, changes its schedule).
#if RENDER_PW_GGX && RENDER_PW_ENV
#define RENDER_PW_KERNEL k_render_ggx_env
#define RENDER_PW_BOX RenderArgsGgxEnvBox
#elif RENDER_PW_GGX
#define RENDER_PW_KERNEL k_render_ggx
#define RENDER_PW_BOX RenderArgsGgxBox
#elif RENDER_PW_ENV
#define RENDER_PW_KERNEL k_render_env
#define RENDER_PW_BOX RenderArgsEnvBox
#else
#define RENDER_PW_KERNEL k_render_pw
#define RENDER_PW_BOX RenderArgsBox
#endif
template <int SHADE_K, int LEAF_K, int NODE_FMT, int THREADS, int MINW, bool STATS, int DIAG = 0, int INNER = 0, int LEAVES = 1, bool LIGHTS = false, int STACK_CAP = 0, int TOPN = 0, int MATH = 0>
__global__ void __launch_bounds__(THREADS, MINW)
RENDER_PW_KERNEL(const RENDER_PW_BOX B)
{
    constexpr bool ENV = RENDER_PW_ENV != 0;
    const RenderArgs& A = B.a[0];                     // what the BVH loop, the queue and the wave set-up use: read once
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    // STACK_CAP > 0: only the first STACK_CAP entries of a lane's stack live in LDS (so that a deep tree does not cost a
    // resident workgroup); the few rays that ever hold more pending nodes keep the rest in global memory (A.stack_overflow).
    // STACK_CAP < 0: a SLIDING WINDOW of -STACK_CAP entries (a power of two) in LDS, addressed circularly: slot k of a lane's
    // stack sits at position k mod window; slots below `wbase` have been moved to global memory.  Pushes and pops inside the
    // BVH loop are plain circular LDS accesses — no comparison, no branch; once per trip a lane whose stack pointer has come
    // within a trip's reach of either end of the window moves four entries out or back in (rare: rays seldom hold more than a
    // dozen pending nodes).  Any tree depth at a fixed LDS cost, and none of the per-access test that made the capped
    // kernel 10 % slower than the plain one on the same tree.
    constexpr bool WINDOW = STACK_CAP < 0;
    constexpr int FM = MATH ? 2 : (DIAG == 3 ? 1 : 0);         // arithmetic level of the shade phase
    // Origin-triangle release (experiment, DIAG 5): a bounce or shadow ray starts ON the triangle its path has just hit and inside
    // that triangle's box, so front-to-back traversal leads it to that leaf first, where it waits for a triangle round only to
    // fail on t < tmin.  When cos(theta_out) * tmin exceeds the rounding between hit point and plane (RenderArgs::skip_base),
    // Moeller-Trumbore cannot accept the origin triangle: a lane found sitting at that leaf when a trip ends moves on at once.
    constexpr bool SKIP = DIAG == 5 && INNER >= 1 && !LIGHTS;
    constexpr int WIN = WINDOW ? -STACK_CAP : 0;
    static_assert(!WINDOW || ((WIN & (WIN - 1)) == 0 && WIN >= 16), "the window wraps by masking and must hold two trips");
    const uint32_t lds_entries = WINDOW ? (uint32_t)WIN + 1u : ((STACK_CAP > 0 && A.stack_entries > (uint32_t)STACK_CAP) ? (uint32_t)STACK_CAP : A.stack_entries);   // WINDOW: entry WIN of a lane's column holds its window base
    const bool deep = WINDOW && A.stack_entries > (uint32_t)WIN;      // wave-uniform: can a stack outgrow the window at all?
    constexpr bool SHARED = NODE_FMT == 10 || NODE_FMT == 12;     // shared-plane records, 15-bit / 30-bit child references
    constexpr uint32_t ENT = SHARED ? 2u : 1u;      // dwords per stack entry: the shared-plane kernel keeps {node, interval}
    LaneStack st;
    st.base = lds_dyn + wave * (lds_entries * 64u * ENT) + lane;
    // the overflow region of this wave: a wave-uniform base (scalar registers) and, where an entry is touched, a 32-bit
    // offset from the entry number and the lane — a per-lane 64-bit pointer held across the kernel cost two vector registers
    // and, at the 96 of five waves per SIMD, spills whose scratch traffic was the 18 GB of fabric writes of round 2's profile
    uint32_t* const ovf = STACK_CAP != 0
        ? A.stack_overflow + (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (THREADS / 64) + wave)) * 64u * ENT * (WINDOW ? A.stack_entries : A.stack_entries - lds_entries) : nullptr;
    const auto push = [&](int at, int v) {
        if (WINDOW) st.push(at & (WIN - 1), v);
        else if (STACK_CAP == 0 || at < (int)lds_entries) st.push(at, v);
        else ovf[(uint32_t)(at - (int)lds_entries) * 64u + lane] = (uint32_t)v;
    };
    const auto pop = [&](int at) -> int {
        if (WINDOW) return st.pop(at & (WIN - 1));
        if (STACK_CAP == 0 || at < (int)lds_entries) return st.pop(at);
        return (int)ovf[(uint32_t)(at - (int)lds_entries) * 64u + lane];
    };
    LaneStack2 st2;                                   // NODE_FMT 3: the same LDS region as stack_entries / 2 groups; NODE_FMT 10: lds_entries 8-byte entries
    st2.base = (uint2*)(lds_dyn + wave * (lds_entries * 64u * ENT)) + lane;
    uint2* const ovf2 = (uint2*)ovf;                  // NODE_FMT 10: the overflow region as 8-byte entries
    DeviceScene sc = A.scene;
    if (NODE_FMT == 3) sc.tris = (const TriRecord*)A.scene.wrecs;      // triangles live in the record array
    const uint2* lds_nodes = (const uint2*)(lds_dyn + (THREADS / 64) * (lds_entries * 64u * ENT));
    if (NODE_FMT == 2) {
        uint4* dst = (uint4*)(lds_dyn + (THREADS / 64) * (lds_entries * 64u));
        const uint4* src = (const uint4*)sc.qnodes;
        for (uint32_t i = threadIdx.x; i < A.n_lds_nodes * 2u; i += THREADS) dst[i] = src[i];
        __syncthreads();
    }
    if (NODE_FMT == 13) {      // experiment: the FIRST 16 bytes of every fp16 node (child 0) staged in LDS, 16 bytes apart; child 1 still comes through the texture path
        uint4* dst = (uint4*)(lds_dyn + (THREADS / 64) * (lds_entries * 64u));
        const uint4* src = (const uint4*)sc.hcnodes;
        for (uint32_t i = threadIdx.x; i < A.n_lds_nodes; i += THREADS) dst[i] = src[2u * i];
        __syncthreads();
    }
    if (NODE_FMT == 14) {      // ... and the whole nodes (32 bytes apart, as in global memory): every node gather from LDS, the texture path sees triangles only
        uint4* dst = (uint4*)(lds_dyn + (THREADS / 64) * (lds_entries * 64u));
        const uint4* src = (const uint4*)sc.hcnodes;
        for (uint32_t i = threadIdx.x; i < A.n_lds_nodes * 2u; i += THREADS) dst[i] = src[i];
        __syncthreads();
    }
    // LCG skip-ahead table behind the stacks (and behind the LDS-staged nodes of NODE_FMT 2 / 13)
    uint32_t* const lcg_skip = lds_dyn + (THREADS / 64) * (lds_entries * 64u * ENT) + (NODE_FMT == 2 || NODE_FMT == 14 ? A.n_lds_nodes * 8u : NODE_FMT == 13 ? A.n_lds_nodes * 4u : 0u);
    if (threadIdx.x < 32u) { lcg_skip[2u * threadIdx.x] = A.lcg_mul[threadIdx.x]; lcg_skip[2u * threadIdx.x + 1u] = A.lcg_add[threadIdx.x]; }
    const WaveBook book = wave_book(lcg_skip + 64u + wave * kBookDwords, lane);
    // TOPN > 0 (experiment): the first TOPN nodes of the tree, breadth first, staged in LDS behind the books — every ray walks them;
    // a node reference with kTopNodeFlag is a position in that copy
    const uint4* const top_lds = (const uint4*)(lcg_skip + 64u + (THREADS / 64) * kBookDwords);
    if (TOPN > 0) {
        uint4* dst = (uint4*)(lcg_skip + 64u + (THREADS / 64) * kBookDwords);
        const uint4* src = (const uint4*)A.scene.top;
        const uint32_t n = (A.scene.n_top < (uint32_t)TOPN ? A.scene.n_top : (uint32_t)TOPN) * 2u;
        const uint32_t* ids = (const uint32_t*)(A.scene.top + kTopNodesMax);        // position -> index in hnodes
        for (uint32_t i = threadIdx.x; i < n; i += THREADS) {
            uint4 v = src[i];
            if ((int)v.w >= 0 && (v.w & kTopNodeFlag) && (v.w & 0xFFFFu) >= (uint32_t)TOPN) v.w = ids[v.w & 0xFFFFu];     // a child past this kernel's cut: back to its index in hnodes
            dst[i] = v;
        }
    }
    __syncthreads();
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int root = sc.n_tris ? ((TOPN > 0 && NODE_FMT == 9) ? (int)kTopNodeFlag : 0) : kSentinel;

    QueueState q; q.shard = A.row_interleave == 3u ? 0u : xcc_id(); q.shards_left = 8; q.res_first = 0; q.res_count = 0; q.grant_g0 = 0; q.grp_pxy = 0xFFFFFFFFu; q.grp_seed = 0; q.skipped = 0; q.free_top = kFoldSlots;
    q.reach_bit = A.row_spans != nullptr ? 0x80000000u : 0u;
    float* const scratch = A.wave_scratch + 3u * (size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (THREADS / 64) + wave)) * ((size_t)kFoldSlots << A.chunk_shift);   // wave-uniform: scalar registers
    unsigned long long n_radiance = 0, n_shadow = 0, n_paths = 0, n_pixels = 0, n_culled = 0;
    unsigned long long n_steps = 0, n_lane_steps = 0, n_rounds = 0, n_lane_rounds = 0;
    uint32_t n_moves = 0;                             // WINDOW: times this wave moved stack entries out of / back into the LDS window
    // STATS only: 100 MHz stamps of this wave's start, of the moment it found the queue empty, and of its end
    unsigned long long t_start = 0, t_drain = 0, t_phase = 0, t_in_shade = 0, t_refill = 0, t_finish = 0, t_newpath = 0, t_mark = 0;
    if (STATS) { t_start = __builtin_amdgcn_s_memrealtime(); t_phase = t_start; }

    LanePixel lp; lp.alive = false; lp.new_path = false; lp.pxy = lp.seed = lp.samples_left = lp.tag = 0; lp.result = mk(0.0f);
    uint32_t pseed = 0;
    int depth = 0;
    f3 att = mk(1.0f);
    // ray in flight (rinv / gro: reciprocal direction and origin, in grid space for quantised nodes)
    f3 ro = mk(0.0f), rd = mk(0.0f, 0.0f, 1.0f), rinv = mk(1.0f), gro = mk(0.0f);
    f3 gfar = mk(0.0f);                               // NODE_FMT 10 only: the root's far plane distances (gro: its near plane distances; rinv: |1 / d| / scale)
    float cur_tn = 0.0f, cur_tf = 0.0f;               // NODE_FMT 10 only: the ray's interval in the box of `node`
    uint32_t tos_iv = 0u;                             // ... and, packed as two fp16, in the box of the stack's top element
    AxisRot rot = {0u, 0u, 0u};                       // NODE_FMT 8 only
    constexpr float rtmin = 0.01f;      // both ray kinds start at 0.01 (:750-757 and :660-672): a literal, not a register
    float rtmax = 0.0f, best_t = 0.0f;
    int best_slot = -1; uint32_t best_prim = 0xFFFFFFFFu;
    int node = kSentinel, sp = 0, tos = kSentinel;
    uint32_t cur_base = 0, cur_list = 0;              // NODE_FMT 3: innermost group of pending children
    bool shadow_ray = false, shadow_hit = false;
    float prev_pdf = 0.0f;                            // LIGHTS (light mode 1) only: pdf of the last sampled direction where a light sample was taken
    bool fin_pending = false;                         // ran out of samples inside the camera cull: its run is finished at the next round's start
    // What the closest-hit left for after the shadow ray (Pending), held while that ray is in flight.  Light mode 0 keeps four values
    // instead of ten: the next bounce's direction (or, for a path that ends on an emitter, the emitter's Ke, which the light
    // sample is added to, :992-1000, 1015-1024) and the light sample's weight; the next bounce's origin is the shadow ray's own
    // origin P (diffuse) or P + R * 1e-4 (conductor, :948) and is recomputed with the closest-hit's operations.
    Pending pd_lights; pd_lights.nxt_org = mk(0.0f); pd_lights.nxt_dir = mk(0.0f, 0.0f, 1.0f); pd_lights.radiance = mk(0.0f); pd_lights.weight = 0.0f; pd_lights.done = true;   // LIGHTS only: the whole record
    f3 keep_dir = mk(0.0f, 0.0f, 1.0f); float keep_weight = 0.0f; bool keep_done = true, keep_metal = false;
    int origin_ref = kSentinel;                       // SKIP: leaf reference of the triangle the ray in flight starts on
    bool skip_now = false, keep_skip = false;         // ... may the ray in flight / the bounce after the shadow ray pass it by

    for (;;) {
        // =========================== shade / regenerate: lanes with no ray in flight ===============
        // launch constants the shade phase needs are read at their points of use (see RenderArgsBox above)
        const auto late = [&]() -> const RenderArgs& { return B.a[opaque_zero()]; };
        if (STATS) { n_rounds += 1; n_lane_rounds += (unsigned long long)popc(vote(lp.alive && node == kSentinel)); t_phase = __builtin_amdgcn_s_memrealtime(); }
        bool segment_done = false, started_shadow = false;
        bool skip_bounce = false;                                     // SKIP: may the bounce that starts in this round pass its origin triangle by
        f3 emission = mk(0.0f);
        Pending pd;                                                   // lives within one shade round (light mode 1: carried in pd_lights)
        if (LIGHTS) pd = pd_lights;
        else { pd.nxt_org = mk(0.0f); pd.nxt_dir = mk(0.0f, 0.0f, 1.0f); pd.radiance = mk(0.0f); pd.weight = 0.0f; pd.done = true; }
        if (lp.alive && node == kSentinel) {
            if (shadow_ray) {                                         // shadow ray back (:1015-1024)
                if (LIGHTS) { if (shadow_hit) pd.radiance = mk(0.0f); }                // the light sample parked there counts only unoccluded
                else {
                    pd.done = keep_done; pd.weight = keep_weight;
                    pd.nxt_dir = keep_dir;
                    pd.nxt_org = keep_metal ? ro + keep_dir * 1e-4f : ro;             // ro is the shadow ray's origin P
                    pd.radiance = keep_done ? keep_dir : mk(0.0f);
                    if (!shadow_hit) pd.radiance = m_madd<FM>(mk(late().light.emission), pd.weight, pd.radiance);
                }
                shadow_ray = false;
                segment_done = true;
                skip_bounce = keep_skip;
            } else {                                                  // radiance ray back
                bool want_shadow = false;
                f3 P, L; float Ldist;
                if (best_slot >= 0) {
#if RENDER_PW_GGX && RENDER_PW_ENV
                    if (LIGHTS) want_shadow = shade_hit_micro<FM, true>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, prev_pdf, pd, P, L, Ldist,
                                                                        [&]() -> const GgxArgs& { return B.g[opaque_zero()]; },
                                                                        [&]() -> const EnvArgs& { return B.e[opaque_zero()]; });
#elif RENDER_PW_GGX
                    if (LIGHTS) want_shadow = shade_hit_micro<FM>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, prev_pdf, pd, P, L, Ldist,
                                                                  [&]() -> const GgxArgs& { return B.g[opaque_zero()]; });
#elif RENDER_PW_ENV
                    if (LIGHTS) want_shadow = shade_hit_lights<FM, true>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, prev_pdf, pd, P, L, Ldist,
                                                                         [&]() -> const EnvArgs& { return B.e[opaque_zero()]; });
#else
                    if (LIGHTS) want_shadow = shade_hit_lights<FM>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, prev_pdf, pd, P, L, Ldist);
#endif
                    else want_shadow = shade_hit<FM, NODE_FMT == 3>(sc, late, ro, rd, best_t, best_slot, depth, pseed, att, emission, pd, P, L, Ldist);
                } else {                                              // __miss__ms :833-847
                    pd.radiance = mk(0.0f); pd.weight = 0.0f; pd.done = true;
#if RENDER_PW_ENV
                    {                                                 // backgroundColor (:568) replaced by the map
                        const EnvArgs& Ev = B.e[opaque_zero()];
                        const EnvMap E = Ev.map;
                        const f3 Le = env_eval(E, rd);
                        if (LIGHTS) {                                 // a BSDF-sampled direction after a light sample: power heuristic against the map's pdf
                            float w = 1.0f;
                            if (depth > 0 && prev_pdf > 0.0f) {
                                const float pe = Ev.p * env_pdf<FM>(E, rd);
                                w = m_div<FM>(prev_pdf * prev_pdf, prev_pdf * prev_pdf + pe * pe);
                            }
                            pd.radiance = att * Le * w;
                        } else {
                            pd.radiance = Le;
                        }
                    }
#endif
                }
                lp.result += emission;                                // :760 (before the radiance term)
                if (SKIP) {
                    // the rays that start at this hit point: cos(theta_out) * tmin against the rounding between P and the triangle's plane
                    const float bound = late().skip_base + kOriginEps * best_t;
                    origin_ref = best_slot >= 0 ? ~best_slot : kSentinel;
                    skip_bounce = best_slot >= 0 && pd.cos_bounce * 0.01f > bound;
                    if (want_shadow) { skip_now = pd.cos_shadow * 0.01f > bound; keep_skip = skip_bounce; }
                }
                if (want_shadow) {
                    if (LIGHTS) pd_lights = pd;
                    else {
                        keep_done = pd.done; keep_weight = pd.weight;
                        keep_dir = pd.done ? pd.radiance : pd.nxt_dir;
                        keep_metal = !pd.done && !(pd.nxt_org.x == P.x && pd.nxt_org.y == P.y && pd.nxt_org.z == P.z);
                    }
                    ro = P; rd = L;
                    if (SHARED) { const RenderArgs& Rs = late(); setup_ray_s(ro, rd, Rs.scene.sspace, rinv, gro, gfar); }
                    else { const RenderArgs& Rs = late(); setup_ray<NODE_FMT>(ro, rd, Rs.scene.grid, Rs.scene.hspace, rinv, gro); }
                    if (NODE_FMT == 8) rot = axis_rot(rinv);
                    rtmax = Ldist - 0.01f; best_t = rtmax; best_slot = -1; best_prim = 0xFFFFFFFFu;
                    node = root; sp = 0; if (WINDOW && deep) { if (SHARED) st2.push(WIN, 0u, 0u); else st.push(WIN, 0); } cur_list = 0u; shadow_ray = true; shadow_hit = false; started_shadow = true;
                    if (SHARED) {       // the ray's interval in the root's box: the root planes' distances are the per-ray constants themselves
                        cur_tn = fmaxf(fmaxf(gro.x, gro.y), fmaxf(gro.z, rtmin)); cur_tf = fminf(fminf(gfar.x, gfar.y), fminf(gfar.z, rtmax));
                        if (!(cur_tn <= cur_tf * kFarWiden)) node = kSentinel;
                    }
                } else {
                    segment_done = true;
                }
            }
        }
        n_shadow += (unsigned long long)popc(vote(started_shadow));
        bool end = false, finished = false;
        if (segment_done) {                                           // raygen :761-778
            if (LIGHTS) lp.result += pd.radiance;                     // light mode 1: already times the throughput
            else add_segment<FM>(lp.result, pd.radiance, att);
            float p = roulette_p<FM>(att);
            if (LIGHTS) p = fminf(p, 1.0f);                           // the 2 cos weight can lift the throughput above 1; a survival probability is <= 1
            const bool rr = rnd(pseed) > p;
            end = pd.done || rr || (uint32_t)depth >= A.maxDepth;
            if (!end) {
                att = roulette_scale<FM>(att, p);
                ro = pd.nxt_org; rd = pd.nxt_dir;
                ++depth;
                if (SKIP) skip_now = skip_bounce;
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
        if (STATS) t_mark = __builtin_amdgcn_s_memrealtime();
        finish_runs(A, q, below, lp, finished, book, scratch);     // before the refill overwrites the lanes' items
        if (STATS) { const unsigned long long now = __builtin_amdgcn_s_memrealtime(); t_finish += now - t_mark; t_mark = now; }

        refill_lanes<STATS, !ENV>(A, late, q, lane, below, lp, lcg_skip, book);
        if (q.skipped != 0u) {      // pixels that cannot reach the scene box: every sample is one radiance segment that misses, one path
            const unsigned long long n = (unsigned long long)q.skipped * A.spp;
            n_radiance += n; n_paths += n; n_culled += n;
            n_pixels += (unsigned long long)q.skipped << A.chunk_shift;
            q.skipped = 0u;
        }
        if (STATS) { const unsigned long long now = __builtin_amdgcn_s_memrealtime(); t_refill += now - t_mark; t_mark = now; }
        if (STATS && t_drain == 0ull && q.shards_left == 0u && q.res_count == 0u) t_drain = __builtin_amdgcn_s_memrealtime();

        bool start_radiance = segment_done && !end;
        uint32_t my_culled = 0u;                                      // per lane: the counters are wave-uniform and must not be touched under divergence
        bool env_culled = false;                                      // ENV: this camera ray misses the scene box; it is the miss of a radiance ray without a traversal
        if (lp.alive && lp.new_path) {                                // camera path start, :727-745
            const RenderArgs& Rc = late();
            const f3 eye = mk(Rc.eye), camU = mk(Rc.U), camV = mk(Rc.V), camW = mk(Rc.W);
            const float fw = (float)(int)Rc.width, fh = (float)(int)Rc.height;
            // camera-ray cull against the scene box (reaches_scene): corners relative to the eye; an empty scene is never reached
            const f3 elo = Rc.scene.n_tris ? mk(Rc.cull_lo) - eye : mk(1.0f), ehi = Rc.scene.n_tris ? mk(Rc.cull_hi) - eye : mk(-1.0f);
            f3 D;
            for (;;) {
                const float jx = rnd(lp.seed);
                const float jy = rnd(lp.seed);
                D = camera_dir<FM>((float)(lp.pxy & 0xFFFFu), (float)(lp.pxy >> 16), jx, jy, fw, fh, camU, camV, camW);
                // a camera ray that cannot reach the scene box: one radiance segment that misses (:833-847 adds nothing to
                // the result, done = true); its path ends here and the lane goes on to its next sample
                if ((lp.tag & (1u << 24)) != 0u || reaches_scene(D, elo, ehi)) break;      // bit 24: every ray of this pixel reaches the box
                if (ENV) { env_culled = true; break; }            // it sees the map: parked at once, shaded as a miss in the next round (one lookup site)
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
                prev_pdf = 0.0f;
                lp.new_path = false;
                start_radiance = true;
                if (SKIP) skip_now = false;                       // a camera ray starts on no triangle
            }
        }
        if (vote(my_culled != 0u) != 0ull) {                           // wave sum of the per-lane counts, bit plane by bit plane
            unsigned long long sum = 0ull;
            for (uint32_t b = 0; vote((my_culled >> b) != 0u) != 0ull; b++) sum += (unsigned long long)popc(vote(((my_culled >> b) & 1u) != 0u)) << b;
            n_radiance += sum; n_paths += sum; n_culled += sum;
        }
        if (STATS) { const unsigned long long now = __builtin_amdgcn_s_memrealtime(); t_newpath += now - t_mark; }
        if (vote(lp.alive) == 0ull) { if (q.shards_left == 0u && q.res_count == 0u && vote(fin_pending) == 0ull) break; else continue; }
        if (start_radiance) {                                         // traceRadiance :750-757
            if (SHARED) { const RenderArgs& Rs = late(); setup_ray_s(ro, rd, Rs.scene.sspace, rinv, gro, gfar); }
            else { const RenderArgs& Rs = late(); setup_ray<NODE_FMT>(ro, rd, Rs.scene.grid, Rs.scene.hspace, rinv, gro); }
            if (NODE_FMT == 8) rot = axis_rot(rinv);
            rtmax = 1e16f; best_t = rtmax; best_slot = -1; best_prim = 0xFFFFFFFFu;
            node = root; sp = 0; if (WINDOW && deep) { if (SHARED) st2.push(WIN, 0u, 0u); else st.push(WIN, 0); } cur_list = 0u; shadow_ray = false;
            if (ENV && env_culled) node = kSentinel;
            if (SHARED) {
                cur_tn = fmaxf(fmaxf(gro.x, gro.y), fmaxf(gro.z, rtmin)); cur_tf = fminf(fminf(gfar.x, gfar.y), fminf(gfar.z, rtmax));
                if (!(cur_tn <= cur_tf * kFarWiden)) node = kSentinel;
            }
        }
        n_radiance += (unsigned long long)popc(vote(start_radiance));
        if (ENV) n_culled += (unsigned long long)popc(vote(env_culled));

        if (STATS) { const unsigned long long now = __builtin_amdgcn_s_memrealtime(); t_in_shade += now - t_phase; t_phase = now; }
        // =========================== traversal: until SHADE_K lanes are parked =====================
        const unsigned long long alive_mask = vote(lp.alive);          // fixed while the wave traverses
        for (;;) {
            const bool act = node != kSentinel;
            const unsigned long long am = vote(act);
            if (am == 0ull) break;
            if (popc(alive_mask & ~am) >= SHADE_K) break;              // parked lanes: scalar arithmetic on the two masks
            if (STATS) { n_steps += 1; n_lane_steps += (unsigned long long)popc(am); }
            if (NODE_FMT == 3) {
                const bool at_inner = act && node >= 0;
                const bool leaf_lane = node < 0;
                const unsigned long long lmask = vote(leaf_lane);
                const bool leaf_round = lmask != 0ull && (LEAF_K <= 1 || popc(lmask) >= LEAF_K || vote(at_inner) == 0ull);
                bool next = false;
                if (at_inner) {
                    uint32_t base;
                    const uint32_t list = wide_visit(sc.wrecs, node, ro, rinv, rtmin, best_t, base);
                    if (list != 0u) {
                        if (cur_list != 0u) { st2.push(sp, cur_base, cur_list); sp++; }
                        cur_base = base; cur_list = list;
                    }
                    next = true;
                }
                if (leaf_round && leaf_lane) {
                    const int slot = ~node;
                    const TriRecord* tp = sc.tris + slot;
                    const float4 r0 = tp->r0, r1 = tp->r1, r2 = tp->r2;
                    float t;
                    const bool ok = tri_test_lazy(ro, rd, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), rtmin, rtmax, t);
                    const uint32_t prim = __float_as_uint(r2.y);
                    if (ok) {
                        if (shadow_ray) { shadow_hit = true; cur_list = 0u; sp = 0; }
                        else if (t < best_t || (t == best_t && prim < best_prim)) { best_t = t; best_slot = slot; best_prim = prim; }
                    }
                    next = true;
                }
                if (next) {
                    if (cur_list == 0u && sp > 0) { sp--; const uint2 g = st2.pop(sp); cur_base = g.x; cur_list = g.y; }
                    if (cur_list != 0u) {
                        const uint32_t nib = cur_list & 15u;
                        cur_list >>= 4;
                        const int idx = (int)(cur_base + (nib & 3u));
                        node = (nib & 4u) ? ~idx : idx;
                    } else {
                        node = kSentinel;
                    }
                }
                continue;
            }
            if constexpr (SHARED) {
                // ---- shared-plane records: one 16-byte gather per visit, the ray's interval carried down and on the stack ----
                static_assert(!SHARED || (INNER >= 1 && STACK_CAP <= 0 && TOPN == 0 && !SKIP), "shared-plane kernel: register stack top, whole or windowed LDS stack");
                constexpr int TRIP = INNER >= 2 ? INNER : 1;
                const auto push8 = [&](int at, int ref, uint32_t iv) { st2.push(WINDOW ? (at & (WIN - 1)) : at, (uint32_t)ref, iv); };
                const auto pop8 = [&](int at, int& ref, uint32_t& iv) { const uint2 e = st2.pop(WINDOW ? (at & (WIN - 1)) : at); ref = (int)e.x; iv = e.y; };
                if (WINDOW && deep) {
                    static_assert(!WINDOW || WIN >= 2 * TRIP + LEAVES + 3, "window too small: moving entries out and back in would alternate");
                    int wbase = (int)st2.pop(WIN).x;
                    for (;;) {
                        const bool out = act && sp + TRIP > wbase + WIN;
                        const bool in = act && wbase > 0 && sp - (TRIP + LEAVES) < wbase;
                        if (vote(out || in) == 0ull) break;
                        n_moves += 1u;
                        if (out) {
#pragma unroll
                            for (int j = 0; j < 4; j++) ovf2[(uint32_t)(wbase + j) * 64u + lane] = st2.pop((wbase + j) & (WIN - 1));
                            wbase += 4;
                        } else if (in) {
                            wbase -= 4;
#pragma unroll
                            for (int j = 0; j < 4; j++) { const uint2 e = ovf2[(uint32_t)(wbase + j) * 64u + lane]; st2.push((wbase + j) & (WIN - 1), e.x, e.y); }
                        }
                        if (out || in) st2.push(WIN, (uint32_t)wbase, 0u);
                    }
                }
#pragma unroll
                for (int visit = 0; visit < TRIP; visit++)
                if ((uint32_t)node < (uint32_t)kSentinel) {
                    const uint4 q = *(const uint4*)((const char*)sc.srecs + (size_t)((uint32_t)node << 4));
                    cur_tf = vmin_raw(cur_tf, best_t * kTieWiden);
                    float n0, f0, n1, f1;
                    slab_s(q.x, q.y, q.z, rinv, gro, gfar, cur_tn, cur_tf, n0, f0, n1, f1);
                    // children: two 16-bit references, bit 15 = triangle (sign-extended: negative, as every leaf reference of this kernel)
                    int c0, c1;
                    if (NODE_FMT == 10) { c0 = (int)(short)(q.w & 0xFFFFu); c1 = (int)q.w >> 16; }
                    else {      // one 30-bit index: child 1 follows child 0 (a triangle is three records); bit 31 / 30: child 0 / 1 is a triangle
                        const uint32_t t = q.w >> 30, base = q.w & kSBaseMask;
                        c0 = (int)(q.w & ~kSLeaf1);
                        c1 = (int)((base + (t & 2u) + 1u) | (t << 31));
                    }
                    const bool h0 = n0 <= f0 * kFarWiden, h1 = n1 <= f1 * kFarWiden;
                    const bool first0 = n0 <= n1;
                    const bool pick0 = h0 && (first0 || !h1);
                    if (h0 && h1) { push8(sp, tos, tos_iv); tos = first0 ? c1 : c0; tos_iv = pack_interval(first0 ? n1 : n0, first0 ? f1 : f0); sp++; }
                    if (h0 || h1) {
                        node = pick0 ? c0 : c1; cur_tn = pick0 ? n0 : n1; cur_tf = pick0 ? f0 : f1;
                    } else {
                        node = sp ? tos : kSentinel;
                        unpack_interval(tos_iv, cur_tn, cur_tf);
                        sp = sp ? sp - 1 : 0;
                        pop8(sp, tos, tos_iv);
                    }
                }
                const bool at_leaf = node < 0;
                const unsigned long long lm = vote(at_leaf);
                if (lm != 0ull && (LEAF_K <= 1 || popc(lm) >= LEAF_K || vote(node >= 0 && node != kSentinel) == 0ull)) {
#pragma unroll
                    for (int leaf = 0; leaf < LEAVES; leaf++)
                    if (node < 0) {
                        const uint4* tp = (const uint4*)((const char*)sc.srecs + (size_t)(((uint32_t)node & (NODE_FMT == 10 ? 0x7FFFu : 0x7FFFFFFFu)) << 4));
                        const uint4 u0 = tp[0], u1 = tp[1], u2 = tp[2];
                        const float4 r0 = make_float4(__uint_as_float(u0.x), __uint_as_float(u0.y), __uint_as_float(u0.z), __uint_as_float(u0.w));
                        const float4 r1 = make_float4(__uint_as_float(u1.x), __uint_as_float(u1.y), __uint_as_float(u1.z), __uint_as_float(u1.w));
                        float t;
                        const bool ok = tri_test_lazy(ro, rd, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, __uint_as_float(u2.x)), rtmin, rtmax, t);
                        const uint32_t prim = u2.y;
                        bool stop = false;
                        if (ok) {
                            if (shadow_ray) { shadow_hit = true; stop = true; }
                            else if (t < best_t || (t == best_t && prim < best_prim)) { best_t = t; best_slot = (int)u2.w; best_prim = prim; }
                        }
                        node = (stop || sp == 0) ? kSentinel : tos;
                        unpack_interval(tos_iv, cur_tn, cur_tf);
                        sp = sp ? sp - 1 : 0;
                        pop8(sp, tos, tos_iv);
                    }
                }
                continue;
            }
            if (WINDOW && deep) {
                // a trip pushes at most TRIP entries (slots sp .. sp + TRIP - 1 must lie inside the window) and pops at most
                // TRIP + LEAVES (down to slot sp - TRIP - LEAVES, which must not have been moved out)
                constexpr int TRIP = INNER >= 2 ? INNER : 1;
                static_assert(!WINDOW || WIN >= 2 * TRIP + LEAVES + 3, "window too small: moving entries out and back in would alternate");
                // slots [0, wbase) of this lane's stack are in global memory; wbase lives in LDS (entry WIN of the lane's column): one
                // conflict-free read per trip instead of a vector register held across the shade phase
                int wbase = st.pop(WIN);
                for (;;) {
                    const bool out = act && sp + TRIP > wbase + WIN;
                    const bool in = act && wbase > 0 && sp - (TRIP + LEAVES) < wbase;
                    if (vote(out || in) == 0ull) break;
                    n_moves += 1u;
                    if (out) {
#pragma unroll
                        for (int j = 0; j < 4; j++) ovf[(uint32_t)(wbase + j) * 64u + lane] = (uint32_t)st.pop((wbase + j) & (WIN - 1));
                        wbase += 4;
                    } else if (in) {
                        wbase -= 4;
#pragma unroll
                        for (int j = 0; j < 4; j++) st.push((wbase + j) & (WIN - 1), (int)ovf[(uint32_t)(wbase + j) * 64u + lane]);
                    }
                    if (out || in) st.push(WIN, wbase);
                }
            }
            // INNER == 2: two node visits per trip through the loop control (a lane that reaches a leaf or runs dry in the
            // first sits out the second)
#pragma unroll
            for (int visit = 0; visit < (INNER >= 2 ? INNER : 1); visit++)
            if ((uint32_t)node < (uint32_t)kSentinel) {
                float n0, f0, n1, f1; int c0, c1;
                if (NODE_FMT == 5) {        // the two-step slab test (p - o) * (1/d): comparison variant
                    const BvhNode* np = sc.nodes + node;
                    const float4 a = np->a, b = np->b, c = np->c;
                    const int4 ch = np->d;
                    c0 = ch.x; c1 = ch.y;
                    float x0 = (a.x - ro.x) * rinv.x, x1 = (a.w - ro.x) * rinv.x;
                    float y0 = (a.y - ro.y) * rinv.y, y1 = (b.x - ro.y) * rinv.y;
                    float z0 = (a.z - ro.z) * rinv.z, z1 = (b.y - ro.z) * rinv.z;
                    n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), rtmin));
                    f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                    float u0 = (b.z - ro.x) * rinv.x, u1 = (c.y - ro.x) * rinv.x;
                    float v0 = (b.w - ro.y) * rinv.y, v1 = (c.z - ro.y) * rinv.y;
                    float w0 = (c.x - ro.z) * rinv.z, w1 = (c.w - ro.z) * rinv.z;
                    n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), rtmin));
                    f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                } else if (NODE_FMT == 0) {
                    // fp32 nodes, slab planes as one full-rate fma each: t = p * (1/d) + (-o/d); lbvh_build.hip's pad_abs
                    // covers the single rounding of -o/d.  32-bit byte offset (scalar base + vector offset addressing; the
                    // scene size limit in pt_set_scene keeps it below 4 GB)
                    const BvhNode* np = (const BvhNode*)((const char*)sc.nodes + (size_t)((uint32_t)node << 6));
                    const float4 a = np->a, b = np->b, c = np->c;
                    const int4 ch = np->d;
                    c0 = ch.x; c1 = ch.y;
                    const float x0 = __builtin_fmaf(a.x, rinv.x, gro.x), x1 = __builtin_fmaf(a.w, rinv.x, gro.x);
                    const float y0 = __builtin_fmaf(a.y, rinv.y, gro.y), y1 = __builtin_fmaf(b.x, rinv.y, gro.y);
                    const float z0 = __builtin_fmaf(a.z, rinv.z, gro.z), z1 = __builtin_fmaf(b.y, rinv.z, gro.z);
                    n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), rtmin));
                    f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                    const float u0 = __builtin_fmaf(b.z, rinv.x, gro.x), u1 = __builtin_fmaf(c.y, rinv.x, gro.x);
                    const float v0 = __builtin_fmaf(b.w, rinv.y, gro.y), v1 = __builtin_fmaf(c.z, rinv.y, gro.y);
                    const float w0 = __builtin_fmaf(c.x, rinv.z, gro.z), w1 = __builtin_fmaf(c.w, rinv.z, gro.z);
                    n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), rtmin));
                    f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                } else if (NODE_FMT == 7) {
                    // fp16 planes, two 16-byte loads; every plane is one v_fma_mix_f32 (the fp16 -> fp32 conversion is part of it)
                    const uint4* np = (const uint4*)((const char*)sc.hnodes + (size_t)((uint32_t)node << 5));
                    const uint4 qa = np[0], qb = np[1];
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    const float x0 = fma_h_lo(qa.x, rinv.x, gro.x), x1 = fma_h_hi(qa.x, rinv.x, gro.x);
                    const float y0 = fma_h_lo(qa.y, rinv.y, gro.y), y1 = fma_h_hi(qa.y, rinv.y, gro.y);
                    const float z0 = fma_h_lo(qa.z, rinv.z, gro.z), z1 = fma_h_hi(qa.z, rinv.z, gro.z);
                    n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), rtmin));
                    f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                    const float u0 = fma_h_lo(qb.x, rinv.x, gro.x), u1 = fma_h_hi(qb.x, rinv.x, gro.x);
                    const float v0 = fma_h_lo(qb.y, rinv.y, gro.y), v1 = fma_h_hi(qb.y, rinv.y, gro.y);
                    const float w0 = fma_h_lo(qb.z, rinv.z, gro.z), w1 = fma_h_hi(qb.z, rinv.z, gro.z);
                    n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), rtmin));
                    f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                } else if (NODE_FMT == 8) {
                    // fp16 planes as NODE_FMT 7; each packed {lo, hi} pair is rotated by the ray's per-axis amount first, so the
                    // low half is always the near plane: 6 rotates replace 12 min / max
                    const uint4* np = (const uint4*)((const char*)sc.hnodes + (size_t)((uint32_t)node << 5));
                    const uint4 qa = np[0], qb = np[1];
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    const uint32_t ax = rot16(qa.x, rot.x), ay = rot16(qa.y, rot.y), az = rot16(qa.z, rot.z);
                    n0 = fmaxf(fmaxf(fma_h_lo(ax, rinv.x, gro.x), fma_h_lo(ay, rinv.y, gro.y)), fmaxf(fma_h_lo(az, rinv.z, gro.z), rtmin));
                    f0 = fminf(fminf(fma_h_hi(ax, rinv.x, gro.x), fma_h_hi(ay, rinv.y, gro.y)), fma_h_hi(az, rinv.z, gro.z)) * kFarWiden;
                    const uint32_t bx = rot16(qb.x, rot.x), by = rot16(qb.y, rot.y), bz = rot16(qb.z, rot.z);
                    n1 = fmaxf(fmaxf(fma_h_lo(bx, rinv.x, gro.x), fma_h_lo(by, rinv.y, gro.y)), fmaxf(fma_h_lo(bz, rinv.z, gro.z), rtmin));
                    f1 = fminf(fminf(fma_h_hi(bx, rinv.x, gro.x), fma_h_hi(by, rinv.y, gro.y)), fma_h_hi(bz, rinv.z, gro.z)) * kFarWiden;
                } else if (NODE_FMT == 9) {
                    // NODE_FMT 8 with the rotate amounts read from the low bits of the plane multipliers (setup_ray)
                    uint4 qa, qb;
                    if (TOPN > 0 && ((uint32_t)node & kTopNodeFlag)) {             // the top of the tree: from LDS
                        const uint4* tp = top_lds + 2u * ((uint32_t)node & 0xFFFFu);
                        qa = tp[0]; qb = tp[1];
                    } else {
                        const uint4* np = (const uint4*)((const char*)sc.hnodes + (size_t)((uint32_t)node << 5));
                        qa = np[0]; qb = np[1];
                    }
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    slab_h9(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_h9(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                } else if (NODE_FMT == 14) {
                    const uint4* np = (const uint4*)((const char*)lds_nodes + (uint32_t)node);
                    const uint4 qa = np[0], qb = np[1];
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    slab_hc(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_hc(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                } else if (NODE_FMT == 13) {
                    // NODE_FMT 11 with child 0's half of the node from LDS (a node's byte offset halved is its place there), child 1's through the texture path
                    const uint4 qa = *(const uint4*)((const char*)lds_nodes + ((uint32_t)node >> 1));
                    const uint4 qb = *(const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node + 16u);
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    slab_hc(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_hc(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                } else if (NODE_FMT == 11) {
                    // fp16 centre / half-extent nodes (pt_device.h): no rotates; child references of inner nodes are byte offsets
                    const uint4* np = (const uint4*)((const char*)sc.hcnodes + (size_t)(uint32_t)node);
                    const uint4 qa = np[0], qb = np[1];
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    slab_hc(qa.x, qa.y, qa.z, rinv, gro, rtmin, n0, f0);
                    slab_hc(qb.x, qb.y, qb.z, rinv, gro, rtmin, n1, f1);
                } else if (NODE_FMT == 6) {
                    // centre / half-extent nodes: near = (c - o)/d - h/|d|, far = (c - o)/d + h/|d|: full-rate arithmetic only,
                    // the |.| is a source modifier
                    const BvhNode* np = (const BvhNode*)((const char*)sc.cnodes + (size_t)((uint32_t)node << 6));
                    const float4 a = np->a, b = np->b, c = np->c;
                    const int4 ch = np->d;
                    c0 = ch.x; c1 = ch.y;
                    const float ax = fabsf(rinv.x), ay = fabsf(rinv.y), az = fabsf(rinv.z);
                    const float cx0 = __builtin_fmaf(a.x, rinv.x, gro.x), hx0 = a.w * ax;
                    const float cy0 = __builtin_fmaf(a.y, rinv.y, gro.y), hy0 = b.x * ay;
                    const float cz0 = __builtin_fmaf(a.z, rinv.z, gro.z), hz0 = b.y * az;
                    n0 = fmaxf(fmaxf(cx0 - hx0, cy0 - hy0), fmaxf(cz0 - hz0, rtmin));
                    f0 = fminf(fminf(cx0 + hx0, cy0 + hy0), cz0 + hz0) * kFarWiden;
                    const float cx1 = __builtin_fmaf(b.z, rinv.x, gro.x), hx1 = c.y * ax;
                    const float cy1 = __builtin_fmaf(b.w, rinv.y, gro.y), hy1 = c.z * ay;
                    const float cz1 = __builtin_fmaf(c.x, rinv.z, gro.z), hz1 = c.w * az;
                    n1 = fmaxf(fmaxf(cx1 - hx1, cy1 - hy1), fmaxf(cz1 - hz1, rtmin));
                    f1 = fminf(fminf(cx1 + hx1, cy1 + hy1), cz1 + hz1) * kFarWiden;
                } else if (NODE_FMT == 4) {
                    // 16-bit grid nodes, one conversion + one fma per plane (the grid's one-cell outward rounding covers the
                    // fma form's error, which is below 0.01 cell)
                    const QNode* np = sc.qnodes + node;
                    const uint4 qa = np->a, qb = np->b;
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    const float x0 = __builtin_fmaf((float)(qa.x & 0xFFFFu), rinv.x, gro.x), x1 = __builtin_fmaf((float)(qa.y >> 16), rinv.x, gro.x);
                    const float y0 = __builtin_fmaf((float)(qa.x >> 16), rinv.y, gro.y), y1 = __builtin_fmaf((float)(qa.z & 0xFFFFu), rinv.y, gro.y);
                    const float z0 = __builtin_fmaf((float)(qa.y & 0xFFFFu), rinv.z, gro.z), z1 = __builtin_fmaf((float)(qa.z >> 16), rinv.z, gro.z);
                    n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), rtmin));
                    f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                    const float u0 = __builtin_fmaf((float)(qb.x & 0xFFFFu), rinv.x, gro.x), u1 = __builtin_fmaf((float)(qb.y >> 16), rinv.x, gro.x);
                    const float v0 = __builtin_fmaf((float)(qb.x >> 16), rinv.y, gro.y), v1 = __builtin_fmaf((float)(qb.z & 0xFFFFu), rinv.y, gro.y);
                    const float w0 = __builtin_fmaf((float)(qb.y & 0xFFFFu), rinv.z, gro.z), w1 = __builtin_fmaf((float)(qb.z >> 16), rinv.z, gro.z);
                    n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), rtmin));
                    f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                } else {
                    uint4 qa, qb;
                    if (NODE_FMT == 2) {
                        const uint2* p = lds_nodes + 4 * node;
                        const uint2 t0 = p[0], t1 = p[1], t2 = p[2], t3 = p[3];
                        qa = make_uint4(t0.x, t0.y, t1.x, t1.y); qb = make_uint4(t2.x, t2.y, t3.x, t3.y);
                    } else {
                        const QNode* np = sc.qnodes + node;
                        qa = np->a; qb = np->b;
                    }
                    c0 = (int)qa.w; c1 = (int)qb.w;
                    float x0 = ((float)(qa.x & 0xFFFFu) - gro.x) * rinv.x, x1 = ((float)(qa.y >> 16) - gro.x) * rinv.x;
                    float y0 = ((float)(qa.x >> 16) - gro.y) * rinv.y, y1 = ((float)(qa.z & 0xFFFFu) - gro.y) * rinv.y;
                    float z0 = ((float)(qa.y & 0xFFFFu) - gro.z) * rinv.z, z1 = ((float)(qa.z >> 16) - gro.z) * rinv.z;
                    n0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), rtmin));
                    f0 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * kFarWiden;
                    float u0 = ((float)(qb.x & 0xFFFFu) - gro.x) * rinv.x, u1 = ((float)(qb.y >> 16) - gro.x) * rinv.x;
                    float v0 = ((float)(qb.x >> 16) - gro.y) * rinv.y, v1 = ((float)(qb.z & 0xFFFFu) - gro.y) * rinv.y;
                    float w0 = ((float)(qb.y & 0xFFFFu) - gro.z) * rinv.z, w1 = ((float)(qb.z >> 16) - gro.z) * rinv.z;
                    n1 = fmaxf(fmaxf(fminf(u0, u1), fminf(v0, v1)), fmaxf(fminf(w0, w1), rtmin));
                    f1 = fminf(fminf(fmaxf(u0, u1), fmaxf(v0, v1)), fmaxf(w0, w1)) * kFarWiden;
                }
                if (DIAG == 1) {
                    float d = n0;
#pragma unroll
                    for (int k = 0; k < 12; k++) asm volatile("v_add_f32 %0, %0, %1" : "+v"(d) : "v"(f0));
                    asm volatile("" :: "v"(d));
                }
                if (DIAG == 2) {
                    const float4* xp = (const float4*)(sc.nodes + node);
    typedef float v4f __attribute__((ext_vector_type(4)));
                    v4f e0, e1;
                    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:32\n\ts_waitcnt vmcnt(0)"
                                 : "=&v"(e0), "=&v"(e1) : "v"(xp) : "memory");
                    asm volatile("" :: "v"(e0), "v"(e1));
                }
                f0 = fminf(f0, best_t * kTieWiden);
                f1 = fminf(f1, best_t * kTieWiden);
                const bool h0 = n0 <= f0, h1 = n1 <= f1;
                if (INNER == 0) {
                    if (h0 && h1) {
                        const bool first0 = n0 <= n1;
                        push(sp, first0 ? c1 : c0);
                        sp++;
                        node = first0 ? c0 : c1;
                    } else if (h0) {
                        node = c0;
                    } else if (h1) {
                        node = c1;
                    } else {
                        if (sp == 0) node = kSentinel; else { sp--; node = pop(sp); }
                    }
                } else {
                    // elements e_1..e_sp, e_sp in `tos`, e_k (k < sp) in LDS slot k
                    const bool first0 = n0 <= n1;
                    const int near_c = (h0 && (first0 || !h1)) ? c0 : c1;
                    const int far_c = first0 ? c1 : c0;
                    if (h0 && h1) { push(sp, tos); tos = far_c; sp++; }
                    if (h0 || h1) {
                        node = near_c;
                    } else {
                        node = sp ? tos : kSentinel;
                        sp = sp ? sp - 1 : 0;
                        tos = pop(sp);
                    }
                }
            }
            if (SKIP) {
                if (skip_now && node == origin_ref) {     // sitting at the triangle the ray started on: it cannot be hit (see SKIP above)
                    node = sp ? tos : kSentinel;
                    sp = sp ? sp - 1 : 0;
                    tos = pop(sp);
                }
            }
            const bool at_leaf = node < 0;       // kSentinel is positive
            const unsigned long long lm = vote(at_leaf);
            if (lm != 0ull && (LEAF_K <= 1 || popc(lm) >= LEAF_K || vote(node >= 0 && node != kSentinel) == 0ull)) {
#pragma unroll
                for (int leaf = 0; leaf < LEAVES; leaf++)          // LEAVES == 2: a lane whose next node is a leaf again tests it in the same round
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
                    if (INNER == 0) {
                        if (stop || sp == 0) node = kSentinel; else { sp--; node = pop(sp); }
                    } else {
                        node = (stop || sp == 0) ? kSentinel : tos;
                        sp = sp ? sp - 1 : 0;
                        tos = pop(sp);
                    }
                }
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&A.counters[0], n_radiance);
        atomicAdd(&A.counters[1], n_shadow);
        atomicAdd(&A.counters[2], n_paths);
        atomicAdd(&A.counters[3], n_pixels);
        atomicAdd(&A.counters[4], n_steps);
        atomicAdd(&A.counters[5], n_lane_steps);
        atomicAdd(&A.counters[6], n_rounds);
        atomicAdd(&A.counters[7], n_lane_rounds);
        if (n_culled) atomicAdd(&A.counters[kCulledCounter], n_culled);
        if (WINDOW && n_moves) atomicAdd(&A.counters[kWindowMoves], (unsigned long long)n_moves);
        if (STATS) {
            const uint32_t w = blockIdx.x * (THREADS / 64) + wave;
            if (w < kMaxTimedWaves) {
                A.counters[8 + 3 * w] = t_start;
                A.counters[8 + 3 * w + 1] = t_drain;
                atomicAdd(&A.counters[8 + 3 * kMaxTimedWaves + 2048], t_in_shade);       // 10 ns units, summed over waves
                atomicAdd(&A.counters[8 + 3 * kMaxTimedWaves + 2049], t_refill);         // ... of which: queue refill,
                atomicAdd(&A.counters[8 + 3 * kMaxTimedWaves + 2050], t_finish);         // finished runs (park / fold / write),
                atomicAdd(&A.counters[8 + 3 * kMaxTimedWaves + 2051], t_newpath);        // camera-path start incl. the cull
                A.counters[8 + 3 * w + 2] = __builtin_amdgcn_s_memrealtime();
            }
        }
    }
}
#undef RENDER_PW_KERNEL
#undef RENDER_PW_BOX
