// QueryCommands.cpp — the query options of acgpt_main: per option its arguments, its parse and its run, and at the end the table
// (QueryCommands.h).  Every option is repeatable and runs once the scene is set and before the first frame; the frames are the
// same with or without it.  A refused value prints the entry's usage line and ends the program with status 2 before any device
// work.  Floats are printed with nine digits: they read back as the same fp32 values.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "QueryCommands.h"

using namespace acgpt;

static const uint32_t kNone = 0xFFFFFFFFu;      // the prim of a record that found nothing, and the padding of a short list

// ---- shared pieces ----------------------------------------------------------------------------------------------------------
// a name inside a JSON string: what would end or break the string becomes '_'
static std::string jsonEscaped(std::string name)
{
    for (size_t k = 0; k < name.size(); k++) if (name[k] == '"' || name[k] == '\\' || (unsigned char)name[k] < 0x20) name[k] = '_';
    return name;
}
// the newmtl name of material `id`, escaped; empty for an id the OBJ does not have
static std::string materialName(const TinyObjWrapper& obj, uint32_t id)
{
    const std::vector<std::string>& names = obj.getMaterialNames();
    return jsonEscaped(id < names.size() ? names[id] : std::string());
}
static void printFiniteOrNull(float v)
{
    if (std::isfinite(v)) printf("%.9g", v); else printf("null");
}

// the camera ray through the centre of pixel (x, y), row 0 at the bottom (the direction of pixel_centre_dir, csrc/image_common.h,
// restated: the same fp32 operations), over pt_render_features' interval
static void cameraRay(const pt_params& p, int x, int y, float* ray)
{
    const float3 eye = make_float3(p.cameraEye.x, p.cameraEye.y, p.cameraEye.z);
    const float3 U = make_float3(p.cameraU.x, p.cameraU.y, p.cameraU.z), V = make_float3(p.cameraV.x, p.cameraV.y, p.cameraV.z),
                 W = make_float3(p.cameraW.x, p.cameraW.y, p.cameraW.z);
    const float dx = 2.0f * (((float)x + 0.5f) / (float)p.width) - 1.0f;
    const float dy = 2.0f * (((float)y + 0.5f) / (float)p.height) - 1.0f;
    const float3 dir = normalize(dx * U + dy * V + W);
    const float r[8] = {eye.x, eye.y, eye.z, dir.x, dir.y, dir.z, 0.01f, 1e16f};
    memcpy(ray, r, sizeof(r));
}
static std::string outsideImage(const char* option, int x, int y, int width, int height)
{
    if (x >= 0 && y >= 0 && x < width && y < height) return std::string();
    return std::string(option) + ": pixel " + std::to_string(x) + "," + std::to_string(y) + " is outside the " + std::to_string(width) + " x " + std::to_string(height) + " image";
}

// the first W floats of every argument's record `v`, back to back
template <typename Arg>
static std::vector<float> records(const std::vector<Arg>& args, size_t W)
{
    std::vector<float> out;
    for (const Arg& a : args) out.insert(out.end(), a.v, a.v + W);
    return out;
}

// n records of W floats in, n result structs out, in one library call
template <typename Result>
static std::vector<Result> queryRecords(PathTracerState& state, const char* what, const float* recs, size_t W, size_t n,
                                        int (*query)(pt_ctx*, const float*, size_t, Result*))
{
    DeviceBuffer d_recs(state.context, n * W * 4, what), d_out(state.context, n * sizeof(Result), what);
    std::vector<Result> out(n);
    d_recs.upload(recs, n * W * 4);
    ptRequire(state.context, query(state.context, d_recs.as<float>(), n, d_out.as<Result>()), what);
    d_out.download(out.data(), n * sizeof(Result));
    return out;
}

// the same for the queries that list up to k results per record and count them all: out holds n * k, counts n
template <typename Result>
static void queryCounted(PathTracerState& state, const char* what, const float* recs, size_t W, size_t n, uint32_t k,
                         int (*query)(pt_ctx*, const float*, size_t, uint32_t, Result*, uint32_t*), std::vector<Result>& out, std::vector<uint32_t>& counts)
{
    DeviceBuffer d_recs(state.context, n * W * 4, what), d_out(state.context, n * k * sizeof(Result), what), d_counts(state.context, n * 4, what);
    out.resize(n * k); counts.resize(n);
    d_recs.upload(recs, n * W * 4);
    ptRequire(state.context, query(state.context, d_recs.as<float>(), n, k, d_out.as<Result>(), d_counts.as<uint32_t>()), what);
    d_out.download(out.data(), n * k * sizeof(Result));
    d_counts.download(counts.data(), n * 4);
}

// --overlap, --overlap-oriented, --intersect: each argument has a record `v` of W floats and a k: 0..8, or kListAll for every
// triangle.  The arguments of one k go through `count` in one call; those that ask for all through `count` for the counts,
// pt_list_offsets for the offsets and `fill` for the lists.  Comes back in the order given: the count and the triangles listed
// (a list shorter than its k ends at kNone).
static const uint32_t kListAll = 9u;
static bool wantsAll(std::string& text)
{
    if (text.size() < 4 || text.compare(text.size() - 4, 4, ",all") != 0) return false;
    text.resize(text.size() - 4);
    return true;
}
struct Listed { std::vector<uint32_t> counts; std::vector<std::vector<uint32_t> > prims; };
template <typename Arg>
static Listed listPerK(PathTracerState& state, const char* what, const std::vector<Arg>& args, size_t W,
                       int (*count)(pt_ctx*, const float*, size_t, uint32_t, uint32_t*, uint32_t*),
                       int (*fill)(pt_ctx*, const float*, size_t, const uint32_t*, uint32_t*, size_t, uint32_t*))
{
    Listed r;
    r.counts.assign(args.size(), 0u); r.prims.resize(args.size());
    for (uint32_t k = 0; k <= kListAll; k++) {
        std::vector<size_t> which;
        std::vector<float> recs;
        for (size_t i = 0; i < args.size(); i++)
            if (args[i].k == k) { which.push_back(i); recs.insert(recs.end(), args[i].v, args[i].v + W); }
        const size_t m = which.size();
        if (m == 0) continue;
        if (k != kListAll) {
            std::vector<uint32_t> c, p;
            queryCounted<uint32_t>(state, what, recs.data(), W, m, k, count, p, c);
            for (size_t j = 0; j < m; j++) {
                r.counts[which[j]] = c[j];
                for (uint32_t e = 0; e < k && p[j * k + e] != kNone; e++) r.prims[which[j]].push_back(p[j * k + e]);
            }
            continue;
        }
        DeviceBuffer d_recs(state.context, m * W * 4, what), d_counts(state.context, m * 4, what), d_offsets(state.context, (m + 1) * 4, what);
        std::vector<uint32_t> offsets(m + 1, 0u);
        uint64_t total = 0;
        d_recs.upload(recs.data(), m * W * 4);
        ptRequire(state.context, count(state.context, d_recs.as<float>(), m, 0u, nullptr, d_counts.as<uint32_t>()), what);
        ptRequire(state.context, pt_list_offsets(state.context, d_counts.as<uint32_t>(), m, d_offsets.as<uint32_t>(), &total), what);
        d_offsets.download(offsets.data(), (m + 1) * 4);
        DeviceBuffer d_prims(state.context, (size_t)total * 4, what);
        std::vector<uint32_t> all((size_t)total, kNone);
        ptRequire(state.context, fill(state.context, d_recs.as<float>(), m, d_offsets.as<uint32_t>(), d_prims.as<uint32_t>(), (size_t)total, nullptr), what);
        d_prims.download(all.data(), (size_t)total * 4);
        for (size_t j = 0; j < m; j++) {
            r.prims[which[j]].assign(all.begin() + offsets[j], all.begin() + offsets[j + 1]);
            r.counts[which[j]] = offsets[j + 1] - offsets[j];
        }
    }
    return r;
}

// --collide, --cast-mesh: the triangles of a second OBJ, as it is, as pt_set_query_mesh takes them; T: how many
static std::vector<float> meshRecords(const std::string& path, size_t& T)
{
    TinyObjWrapper mesh(path);
    const std::vector<float> v = mesh.getVerticesFloat();
    const std::vector<uint32_t> idx = mesh.getIndexBuffer();
    T = idx.size() / 3;
    std::vector<float> recs(T * 12, 0.0f);
    for (size_t k = 0; k < T * 3; k++) for (int c = 0; c < 3; c++) recs[k * 4 + c] = v[(size_t)idx[k] * 4 + c];
    return recs;
}

// ---- --pick x,y ---------------------------------------------------------------------------------------------------------------
// What lies under pixel (x, y), row 0 at the bottom: the closest hit of the camera ray through the pixel's centre (pt_query_closest
// in one call; the ray of pt_render_features), one JSON line each:
// {"pick": [x, y], "hit": true, "t": .., "prim": .., "material": "<newmtl name>", "position": [eye + t * dir], "normal": [..]}, on a
// miss {"pick": [x, y], "hit": false}.  A pixel outside the image is refused with exit status 2.
static std::vector<int2> g_picks;
static bool parsePick(const char* text)
{
    int2 px;
    if (sscanf(text, "%d,%d", &px.x, &px.y) != 2) return false;
    g_picks.push_back(px);
    return true;
}
static std::string checkPick(int width, int height)
{
    for (const int2& px : g_picks) {
        const std::string why = outsideImage("--pick", px.x, px.y, width, height);
        if (!why.empty()) return why;
    }
    return std::string();
}
static void runPick(PathTracerState& state, const TinyObjWrapper& obj)
{
    const size_t n = g_picks.size();
    std::vector<float> rays(n * 8);
    for (size_t i = 0; i < n; i++) cameraRay(state.params, g_picks[i].x, g_picks[i].y, &rays[8 * i]);
    const std::vector<pt_hit> hits = queryRecords<pt_hit>(state, "pick", rays.data(), 8, n, pt_query_closest);
    for (size_t i = 0; i < n; i++) {
        const pt_hit& h = hits[i];
        if (h.prim == kNone) { printf("{\"pick\": [%d, %d], \"hit\": false}\n", g_picks[i].x, g_picks[i].y); continue; }
        const float* r = &rays[8 * i];
        printf("{\"pick\": [%d, %d], \"hit\": true, \"t\": %.9g, \"prim\": %u, \"material\": \"%s\", \"position\": [%.9g, %.9g, %.9g], \"normal\": [%.9g, %.9g, %.9g]}\n",
               g_picks[i].x, g_picks[i].y, h.t, h.prim, materialName(obj, h.material).c_str(), r[0] + h.t * r[3], r[1] + h.t * r[4], r[2] + h.t * r[5], h.nx, h.ny, h.nz);
    }
    fflush(stdout);
}

// ---- --pick-all x,y[,k] -------------------------------------------------------------------------------------------------------
// --pick's camera ray, and everything it goes through (pt_query_multi with counts, one call at the largest k asked for): one JSON
// line each, {"pick_all": [x, y], "count": <triangles the ray crosses inside the interval>, "hits": [<the first k of them in order of
// (t, prim), k = 1..8, default 4, each with --pick's fields t, prim, material, position, normal>]}.  A pixel outside the image or a k
// outside 1..8 is refused with exit status 2.
struct PickAll { int x, y, k; };
static std::vector<PickAll> g_pickAlls;
static_assert(PT_QUERY_MULTI_MAX == 8, "the usage line of --pick-all names the range");
static bool parsePickAll(const char* text)
{
    PickAll pa; pa.k = 4;
    const int got = sscanf(text, "%d,%d,%d", &pa.x, &pa.y, &pa.k);
    if (got < 2 || pa.k < 1 || pa.k > PT_QUERY_MULTI_MAX) return false;
    g_pickAlls.push_back(pa);
    return true;
}
static std::string checkPickAll(int width, int height)
{
    for (const PickAll& px : g_pickAlls) {
        const std::string why = outsideImage("--pick-all", px.x, px.y, width, height);
        if (!why.empty()) return why;
    }
    return std::string();
}
static void runPickAll(PathTracerState& state, const TinyObjWrapper& obj)
{
    const size_t n = g_pickAlls.size();
    uint32_t kmax = 1;
    std::vector<float> rays(n * 8);
    for (size_t i = 0; i < n; i++) {
        cameraRay(state.params, g_pickAlls[i].x, g_pickAlls[i].y, &rays[8 * i]);
        if ((uint32_t)g_pickAlls[i].k > kmax) kmax = (uint32_t)g_pickAlls[i].k;
    }
    std::vector<pt_hit> hits;
    std::vector<uint32_t> counts;
    queryCounted<pt_hit>(state, "pick-all", rays.data(), 8, n, kmax, pt_query_multi, hits, counts);
    for (size_t i = 0; i < n; i++) {
        const float* r = &rays[8 * i];
        printf("{\"pick_all\": [%d, %d], \"count\": %u, \"hits\": [", g_pickAlls[i].x, g_pickAlls[i].y, counts[i]);
        for (int j = 0; j < g_pickAlls[i].k; j++) {
            const pt_hit& h = hits[i * kmax + (size_t)j];
            if (h.prim == kNone) break;
            printf("%s{\"t\": %.9g, \"prim\": %u, \"material\": \"%s\", \"position\": [%.9g, %.9g, %.9g], \"normal\": [%.9g, %.9g, %.9g]}", j ? ", " : "",
                   h.t, h.prim, materialName(obj, h.material).c_str(), r[0] + h.t * r[3], r[1] + h.t * r[4], r[2] + h.t * r[5], h.nx, h.ny, h.nz);
        }
        printf("]}\n");
    }
    fflush(stdout);
}

// ---- --nearest x,y,z[,radius] -------------------------------------------------------------------------------------------------
// The closest surface point to (x, y, z) within radius (no limit if not given), by pt_query_nearest in one call, one JSON line each:
// {"nearest": [x, y, z], "found": true, "distance": .., "triangle": .., "material": "<newmtl name>", "point": [..], "u": .., "v": ..}
// (u, v the weights of the triangle's second and third vertex at the point), {"nearest": [x, y, z], "found": false} if nothing lies
// within the radius.  A coordinate that is not finite or a radius that is negative or no number is refused with exit status 2.
static std::vector<float4> g_nearest;
static bool parseNearest(const char* text)
{
    float4 q = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
    const int got = sscanf(text, "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
    if (got < 3 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 0.0f)) return false;
    g_nearest.push_back(q);
    return true;
}
static void runNearest(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<pt_nearest> out = queryRecords<pt_nearest>(state, "nearest", (const float*)g_nearest.data(), 4, g_nearest.size(), pt_query_nearest);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_nearest& r = out[i];
        const float4& q = g_nearest[i];
        if (r.prim == kNone) { printf("{\"nearest\": [%.9g, %.9g, %.9g], \"found\": false}\n", q.x, q.y, q.z); continue; }
        printf("{\"nearest\": [%.9g, %.9g, %.9g], \"found\": true, \"distance\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}\n",
               q.x, q.y, q.z, r.distance, r.prim, materialName(obj, r.material).c_str(), r.cx, r.cy, r.cz, r.u, r.v);
    }
    fflush(stdout);
}

// ---- --nearest-k x,y,z,k[,radius] ---------------------------------------------------------------------------------------------
// The k closest triangles (k = 1..8) of the point within the radius (default: no limit) in order, by pt_query_nearest_k with counts
// in one call per k, one JSON line each, in the order given: {"nearest_k": [x, y, z], "k": k, "count": <triangles within the
// radius>, "list": [{"distance": .., "triangle": .., "material": "<newmtl name>", "point": [..], "u": .., "v": ..} per listed
// triangle, closest first]}.  A coordinate that is not finite, a k outside 1..8 or a radius that is negative or no number is
// refused with exit status 2.
struct NearestKPoint { float4 q; uint32_t k; };
static std::vector<NearestKPoint> g_nearestKs;
static bool parseNearestK(const char* text)
{
    NearestKPoint p = {make_float4(0.0f, 0.0f, 0.0f, INFINITY), 0u};
    float kf = 0.0f;
    const int got = sscanf(text, "%f,%f,%f,%f,%f", &p.q.x, &p.q.y, &p.q.z, &kf, &p.q.w);
    if (got < 4 || !std::isfinite(p.q.x) || !std::isfinite(p.q.y) || !std::isfinite(p.q.z) || !(kf >= 1.0f && kf <= (float)PT_QUERY_NEAREST_MAX) || kf != std::floor(kf) || !(p.q.w >= 0.0f))
        return false;
    p.k = (uint32_t)kf;
    g_nearestKs.push_back(p);
    return true;
}
static void runNearestK(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<NearestKPoint>& points = g_nearestKs;
    std::vector<std::string> lines(points.size());
    for (uint32_t k = 1; k <= PT_QUERY_NEAREST_MAX; k++) {
        std::vector<size_t> which;
        std::vector<float4> in;
        for (size_t i = 0; i < points.size(); i++) if (points[i].k == k) { which.push_back(i); in.push_back(points[i].q); }
        const size_t n = in.size();
        if (n == 0) continue;
        std::vector<pt_nearest> out;
        std::vector<uint32_t> counts;
        queryCounted<pt_nearest>(state, "nearest-k", (const float*)in.data(), 4, n, k, pt_query_nearest_k, out, counts);
        char buf[512];
        for (size_t i = 0; i < n; i++) {
            const float4& q = in[i];
            snprintf(buf, sizeof buf, "{\"nearest_k\": [%.9g, %.9g, %.9g], \"k\": %u, \"count\": %u, \"list\": [", q.x, q.y, q.z, k, counts[i]);
            std::string line = buf;
            for (uint32_t j = 0; j < k; j++) {
                const pt_nearest& r = out[i * k + j];
                if (r.prim == kNone) break;
                snprintf(buf, sizeof buf, "%s{\"distance\": %.9g, \"triangle\": %u, \"material\": \"", j ? ", " : "", r.distance, r.prim);
                line += buf;
                line += materialName(obj, r.material);
                snprintf(buf, sizeof buf, "\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}", r.cx, r.cy, r.cz, r.u, r.v);
                line += buf;
            }
            lines[which[i]] = line + "]}";
        }
    }
    for (const std::string& l : lines) printf("%s\n", l.c_str());
    fflush(stdout);
}

// ---- --within x,y,z,radius ----------------------------------------------------------------------------------------------------
// Whether anything of the scene lies within the radius of the point, all in one call of pt_query_within_any, one JSON line each:
// {"within": [x, y, z], "radius": r, "hit": true or false}.  The refusals of --nearest-k.
static std::vector<float4> g_withins;
static bool parseWithin(const char* text)
{
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int got = sscanf(text, "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
    if (got < 4 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 0.0f)) return false;
    g_withins.push_back(q);
    return true;
}
static void runWithin(PathTracerState& state, const TinyObjWrapper&)
{
    const std::vector<float4>& points = g_withins;
    const std::vector<uint8_t> hit = queryRecords<uint8_t>(state, "within", (const float*)points.data(), 4, points.size(), pt_query_within_any);
    for (size_t i = 0; i < hit.size(); i++)
        printf("{\"within\": [%.9g, %.9g, %.9g], \"radius\": %.9g, \"hit\": %s}\n", points[i].x, points[i].y, points[i].z, points[i].w, hit[i] ? "true" : "false");
    fflush(stdout);
}

// ---- --winding x,y,z[,beta] ---------------------------------------------------------------------------------------------------
// The generalised winding number of the mesh at the point (pt_query_winding, one call per point: each has its own beta, in .w;
// beta >= 1, default PT_WINDING_BETA_DEFAULT, inf for the exact sum), one JSON line each: {"winding": [x, y, z], "beta": b, "w": ..,
// "inside": true or false} (inside: w > 0.5; an infinite beta is printed as the string "inf").  A coordinate that is not finite or
// a beta below 1 or no number is refused with exit status 2.
static std::vector<float4> g_windings;
static bool parseWinding(const char* text)
{
    float4 q = make_float4(0.0f, 0.0f, 0.0f, PT_WINDING_BETA_DEFAULT);
    const int got = sscanf(text, "%f,%f,%f,%f", &q.x, &q.y, &q.z, &q.w);
    if (got < 3 || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z) || !(q.w >= 1.0f)) return false;
    g_windings.push_back(q);
    return true;
}
static void runWinding(PathTracerState& state, const TinyObjWrapper&)
{
    const std::vector<float4>& points = g_windings;
    DeviceBuffer d_point(state.context, 16, "winding"), d_w(state.context, 4, "winding");
    std::vector<float> w(points.size(), 0.0f);
    for (size_t i = 0; i < points.size(); i++) {
        d_point.upload(&points[i], 16);
        ptRequire(state.context, pt_query_winding(state.context, d_point.as<float>(), 1, points[i].w, d_w.as<float>()), "winding");
        d_w.download(&w[i], 4);
    }
    for (size_t i = 0; i < points.size(); i++) {
        char beta[32];
        if (std::isinf(points[i].w)) snprintf(beta, sizeof(beta), "\"inf\""); else snprintf(beta, sizeof(beta), "%.9g", points[i].w);
        printf("{\"winding\": [%.9g, %.9g, %.9g], \"beta\": %s, \"w\": %.9g, \"inside\": %s}\n", points[i].x, points[i].y, points[i].z, beta, w[i],
               w[i] > 0.5f ? "true" : "false");
    }
    fflush(stdout);
}

// ---- --clearance x0,y0,z0,x1,y1,z1[,radius] -----------------------------------------------------------------------------------
// How far the segment from (x0, y0, z0) to (x1, y1, z1) is from the scene and where the two come closest, all in one call of
// pt_query_segments with no limit on the distance, one JSON line each: {"clearance": [the six coordinates], "radius": r, "found":
// true, "distance": .., "clear": <distance - radius: negative where a capsule of that radius penetrates>, "triangle": ..,
// "material": "<newmtl name>", "s": <parameter of the closest point on the segment>, "feature": <0, 1 an end; 2, 3, 4 an edge of the
// triangle; 5 the segment crosses it>, "on_segment": [..], "point": [<on the triangle>]}, {"clearance": [..], "radius": r, "found":
// false} for a scene without triangles.  radius defaults to 0.  A coordinate that is not finite or a radius that is negative or no
// number is refused with exit status 2.
struct ClearanceSegment { float v[8]; float radius; };
static std::vector<ClearanceSegment> g_clearances;
static bool parseClearance(const char* text)
{
    ClearanceSegment cs = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f};
    float* g = cs.v;
    const int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f", &g[0], &g[1], &g[2], &g[4], &g[5], &g[6], &cs.radius);
    bool fine = got >= 6 && cs.radius >= 0.0f && std::isfinite(cs.radius);
    for (int k = 0; k < 7; k++) if (k != 3 && !std::isfinite(g[k])) fine = false;
    if (!fine) return false;
    g_clearances.push_back(cs);
    return true;
}
static void runClearance(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<ClearanceSegment>& segs = g_clearances;
    const std::vector<pt_segment_hit> out = queryRecords<pt_segment_hit>(state, "clearance", records(segs, 8).data(), 8, segs.size(), pt_query_segments);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_segment_hit& r = out[i];
        const float* g = segs[i].v;
        printf("{\"clearance\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"radius\": %.9g, ", g[0], g[1], g[2], g[4], g[5], g[6], segs[i].radius);
        if (r.prim == kNone) { printf("\"found\": false}\n"); continue; }
        const float px = g[0] + (g[4] - g[0]) * r.s, py = g[1] + (g[5] - g[1]) * r.s, pz = g[2] + (g[6] - g[2]) * r.s;
        printf("\"found\": true, \"distance\": %.9g, \"clear\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"s\": %.9g, \"feature\": %d, \"on_segment\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.distance, r.distance - segs[i].radius, r.prim, materialName(obj, r.material).c_str(), r.s, (int)r.feature, px, py, pz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// ---- --tri-distance x0,y0,z0,x1,y1,z1,x2,y2,z2[,radius] -----------------------------------------------------------------------
// How far the triangle with these vertices is from the scene and where the two come closest, all in one call of
// pt_query_triangle_distance, one JSON line each: {"tri_distance": [the nine coordinates], "radius": <radius or null>, "found": true,
// "distance": .., "triangle": .., "material": "<newmtl name>", "feature": <0..2 a vertex of the query; 3..5 a vertex of the scene
// triangle; 6..14 an edge pair; 15..17 a query edge crosses the scene triangle; 18..20 a scene edge crosses the query>, "on_query":
// [<on the query triangle>], "point": [<on the scene triangle>]}, {"tri_distance": [..], "radius": .., "found": false} if nothing
// lies within the radius (default: no limit).  Fewer than nine or more than ten numbers, a coordinate that is not finite or a radius
// that is negative or no number is refused with exit status 2.
struct DistanceTriangle { float v[12]; bool limited; };
static std::vector<DistanceTriangle> g_triDistances;
static bool parseTriDistance(const char* text)
{
    DistanceTriangle dt = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, false};
    float* g = dt.v;
    int used = 0;
    int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f,%f%n", &g[0], &g[1], &g[2], &g[4], &g[5], &g[6], &g[8], &g[9], &g[10], &used);
    bool fine = got == 9;
    if (fine && text[used] != '\0') {                  // a tenth number, the radius, and nothing behind it
        int more = 0;
        fine = sscanf(text + used, ",%f%n", &g[3], &more) == 1 && text[used + more] == '\0' && g[3] >= 0.0f;
        dt.limited = true;
    }
    for (int k = 0; k < 11; k++) if (k != 3 && k != 7 && !std::isfinite(g[k])) fine = false;
    if (!fine) return false;
    g_triDistances.push_back(dt);
    return true;
}
static void runTriDistance(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<DistanceTriangle>& tris = g_triDistances;
    const std::vector<pt_triangle_distance_hit> out =
        queryRecords<pt_triangle_distance_hit>(state, "tri-distance", records(tris, 12).data(), 12, tris.size(), pt_query_triangle_distance);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_triangle_distance_hit& r = out[i];
        const float* g = tris[i].v;
        printf("{\"tri_distance\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"radius\": ", g[0], g[1], g[2], g[4], g[5], g[6], g[8], g[9], g[10]);
        if (tris[i].limited && std::isfinite(g[3])) printf("%.9g, ", g[3]); else printf("null, ");
        if (r.prim == kNone) { printf("\"found\": false}\n"); continue; }
        printf("\"found\": true, \"distance\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"feature\": %d, \"on_query\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.distance, r.prim, materialName(obj, r.material).c_str(), (int)r.feature, r.qx, r.qy, r.qz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// ---- --collide mesh.obj[,tx,ty,tz[,radius]] -----------------------------------------------------------------------------------
// A second OBJ as the query mesh of the posed-mesh queries (pt_set_query_mesh), moved by the translation; one JSON line each: does
// it touch the scene (pt_query_poses_any), the first mesh triangle that does, and with a radius the closest pair
// (pt_query_poses_distance).  No file name, a translation that is not finite, a radius that is negative or text behind the last
// number is refused with exit status 2.
struct CollideMesh { std::string path; float t[3]; float radius; bool limited; };
static std::vector<CollideMesh> g_collides;
static bool parseCollide(const char* value)
{
    CollideMesh cm = {std::string(), {0.0f, 0.0f, 0.0f}, 0.0f, false};
    const std::string text = value;
    const size_t comma = text.find(',');
    cm.path = text.substr(0, comma);
    bool fine = !cm.path.empty();
    if (fine && comma != std::string::npos) {
        int used = 0;
        const char* rest = text.c_str() + comma;
        fine = sscanf(rest, ",%f,%f,%f%n", &cm.t[0], &cm.t[1], &cm.t[2], &used) == 3;
        if (fine && rest[used] != '\0') {               // a fourth number, the radius, and nothing behind it
            int more = 0;
            fine = sscanf(rest + used, ",%f%n", &cm.radius, &more) == 1 && rest[used + more] == '\0' && cm.radius >= 0.0f;
            cm.limited = true;
        }
        for (int k = 0; k < 3; k++) if (!std::isfinite(cm.t[k])) fine = false;
    }
    if (!fine) return false;
    g_collides.push_back(cm);
    return true;
}
static void runCollide(PathTracerState& state, const TinyObjWrapper&)
{
    for (const CollideMesh& m : g_collides) {
        size_t T = 0;
        const std::vector<float> recs = meshRecords(m.path, T);
        const float pose[12] = {1.0f, 0.0f, 0.0f, m.t[0], 0.0f, 1.0f, 0.0f, m.t[1], 0.0f, 0.0f, 1.0f, m.t[2]};
        uint8_t hit = 0; uint32_t first = kNone;
        pt_pose_distance_hit r;
        if (T == 0) throw Exception("collide: the mesh has no triangles");
        ptRequire(state.context, pt_set_query_mesh(state.context, recs.data(), T), "collide");
        DeviceBuffer d_pose(state.context, 48, "collide"), d_hit(state.context, 16, "collide"), d_first(state.context, 16, "collide"), d_out(state.context, sizeof(r), "collide");
        d_pose.upload(pose, 48);
        ptRequire(state.context, pt_query_poses_any(state.context, d_pose.as<float>(), 1, d_hit.as<uint8_t>(), d_first.as<uint32_t>()), "collide");
        d_hit.download(&hit, 1); d_first.download(&first, 4);
        if (m.limited) {
            ptRequire(state.context, pt_query_poses_distance(state.context, d_pose.as<float>(), 1, m.radius, d_out.as<pt_pose_distance_hit>()), "collide");
            d_out.download(&r, sizeof(r));
        }
        printf("{\"collide\": {\"mesh\": \"%s\", \"triangles\": %zu, \"translation\": [%.9g, %.9g, %.9g], \"hit\": %d, \"first\": %lld", jsonEscaped(m.path).c_str(), T, m.t[0], m.t[1], m.t[2],
               (int)hit, first == kNone ? -1ll : (long long)first);
        if (m.limited) {
            const bool found = r.prim != kNone;
            printf(", \"radius\": %.9g, \"found\": %s, \"distance\": %.9g, \"query_triangle\": %lld, \"prim\": %lld, \"feature\": %d, \"on_query\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]",
                   m.radius, found ? "true" : "false", r.distance, found ? (long long)r.query_triangle : -1ll, found ? (long long)r.prim : -1ll, (int)r.feature, r.qx, r.qy, r.qz,
                   r.cx, r.cy, r.cz);
        }
        printf("}}\n");
    }
    fflush(stdout);
}

// ---- --overlap cx,cy,cz,hx,hy,hz[,k|,all] and --overlap-oriented cx,cy,cz,hx,hy,hz,qw,qx,qy,qz[,k|,all] ------------------------------
// --overlap: the triangles that overlap the axis-aligned box of centre (cx, cy, cz) and half extent (hx, hy, hz), by pt_query_overlap
// in one call per k, one JSON line each: {"overlap": [cx, cy, cz, hx, hy, hz], "count": <triangles that overlap the box>,
// "triangles": [<the k lowest indices among them, k = 0..8, default 8>], "materials": ["<newmtl name>" per listed triangle]}.  A value
// that is not finite, a negative half extent or a k outside 0..8 is refused with exit status 2.  With "all" in place of k the line
// is the same and "triangles" holds every overlapping triangle, ascending: pt_query_overlap counts, pt_list_offsets makes the
// offsets, pt_query_overlap_lists fills the list.
// --overlap-oriented: the same for the oriented box whose axes are the columns of the rotation of the quaternion (qw, qx, qy, qz),
// normalised in double here, by pt_query_overlap_oriented and pt_query_overlap_oriented_lists on records of 16 floats:
// {"overlap_oriented": [the ten numbers, the quaternion normalised], "count", "triangles", "materials"}.
struct OverlapBox { float v[16]; uint32_t k; double arg[10]; };
static std::vector<OverlapBox> g_overlaps, g_orientedOverlaps;
static bool parseOverlap(const char* value)
{
    OverlapBox b = {{0.0f}, 8u, {0.0}};
    int k = 8;
    std::string text = value;
    const bool all = wantsAll(text);
    const int got = sscanf(text.c_str(), "%f,%f,%f,%f,%f,%f,%d", &b.v[0], &b.v[1], &b.v[2], &b.v[3], &b.v[4], &b.v[5], &k);
    bool ok = (all ? got == 6 : got >= 6) && k >= 0 && k <= 8;
    if (all) k = (int)kListAll;
    for (int j = 0; j < 6; j++) ok = ok && std::isfinite(b.v[j]) && (j < 3 || b.v[j] >= 0.0f);
    if (!ok) return false;
    b.k = (uint32_t)k;
    g_overlaps.push_back(b);
    return true;
}
static bool parseOverlapOriented(const char* value)
{
    OverlapBox b = {{0.0f}, 8u, {0.0}};
    int k = 8;
    std::string text = value;
    const bool all = wantsAll(text);
    double* q = b.arg;
    const int got = sscanf(text.c_str(), "%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%d", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8], &q[9], &k);
    bool ok = (all ? got == 10 : got >= 10) && k >= 0 && k <= 8;
    if (all) k = (int)kListAll;
    for (int j = 0; j < 10; j++) ok = ok && std::isfinite((float)q[j]) && (j < 3 || j >= 6 || (float)q[j] >= 0.0f);
    const double len = std::sqrt(q[6] * q[6] + q[7] * q[7] + q[8] * q[8] + q[9] * q[9]);
    ok = ok && std::isfinite(len) && len > 0.0;
    if (!ok) return false;
    // the quaternion is normalised in double; the rotation it stands for, local -> world, rounded to float once per entry
    for (int j = 6; j < 10; j++) q[j] /= len;
    const double w = q[6], x = q[7], y = q[8], z = q[9];
    const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int row = 0; row < 3; row++) {
        for (int col = 0; col < 3; col++) b.v[4 * row + col] = (float)r[3 * row + col];
        b.v[4 * row + 3] = (float)q[row];
        b.v[12 + row] = (float)q[3 + row];
    }
    b.k = (uint32_t)k;
    g_orientedOverlaps.push_back(b);
    return true;
}
static void overlapBoxes(PathTracerState& state, const TinyObjWrapper& obj, const std::vector<OverlapBox>& boxes, bool oriented)
{
    const Listed found = oriented ? listPerK(state, "overlap-oriented", boxes, 16, pt_query_overlap_oriented, pt_query_overlap_oriented_lists)
                                  : listPerK(state, "overlap", boxes, 8, pt_query_overlap, pt_query_overlap_lists);
    const std::vector<uint32_t> mats = obj.getMaterialIndices();
    for (size_t i = 0; i < boxes.size(); i++) {
        const float* b = boxes[i].v;
        if (oriented) {
            const double* q = boxes[i].arg;
            printf("{\"overlap_oriented\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.17g, %.17g, %.17g, %.17g], \"count\": %u, \"triangles\": [", q[0], q[1], q[2], q[3],
                   q[4], q[5], q[6], q[7], q[8], q[9], found.counts[i]);
        } else
            printf("{\"overlap\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"count\": %u, \"triangles\": [", b[0], b[1], b[2], b[3], b[4], b[5], found.counts[i]);
        std::string mat_list;
        bool first = true;
        for (uint32_t t : found.prims[i]) {
            if (t == kNone) break;
            printf("%s%u", first ? "" : ", ", t);
            mat_list += std::string(first ? "" : ", ") + "\"" + materialName(obj, t < mats.size() ? mats[t] : kNone) + "\"";
            first = false;
        }
        printf("], \"materials\": [%s]}\n", mat_list.c_str());
    }
    fflush(stdout);
}
static void runOverlap(PathTracerState& state, const TinyObjWrapper& obj) { overlapBoxes(state, obj, g_overlaps, false); }
static void runOverlapOriented(PathTracerState& state, const TinyObjWrapper& obj) { overlapBoxes(state, obj, g_orientedOverlaps, true); }

// ---- --intersect x0,y0,z0,x1,y1,z1,x2,y2,z2[,k|,all] --------------------------------------------------------------------------
// The scene triangles that intersect the triangle of these three vertices, by pt_query_triangles in one call per k, one JSON line
// each: {"intersect": [the nine coordinates], "count": <scene triangles that intersect it>, "triangles": [<the k lowest indices among
// them, k = 0..8, default 8>]}.  A coordinate that is not finite or a k outside 0..8 is refused with exit status 2.  "all" in place
// of k lists every intersecting scene triangle, through pt_query_triangles_lists as --overlap does.
struct IntersectTri { float v[12]; uint32_t k; };
static std::vector<IntersectTri> g_intersects;
static bool parseIntersect(const char* value)
{
    IntersectTri t = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 8u};
    int k = 8;
    float* v = t.v;
    std::string text = value;
    const bool all = wantsAll(text);
    const int got = sscanf(text.c_str(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%d", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &k);
    bool ok = (all ? got == 9 : got >= 9) && k >= 0 && k <= 8;
    if (all) k = (int)kListAll;
    for (int j = 0; j < 12; j++) ok = ok && std::isfinite(v[j]);
    if (!ok) return false;
    t.k = (uint32_t)k;
    g_intersects.push_back(t);
    return true;
}
static void runIntersect(PathTracerState& state, const TinyObjWrapper&)
{
    const Listed found = listPerK(state, "intersect", g_intersects, 12, pt_query_triangles, pt_query_triangles_lists);
    for (size_t i = 0; i < g_intersects.size(); i++) {
        const float* a = g_intersects[i].v;
        printf("{\"intersect\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"count\": %u, \"triangles\": [", a[0], a[1], a[2], a[4], a[5], a[6], a[8],
               a[9], a[10], found.counts[i]);
        for (size_t e = 0; e < found.prims[i].size(); e++) printf("%s%u", e ? ", " : "", found.prims[i][e]);
        printf("]}\n");
    }
    fflush(stdout);
}

// ---- --sweep ox,oy,oz,dx,dy,dz,r[,tmax] ---------------------------------------------------------------------------------------
// How far the sphere of radius r whose centre starts at o travels along d before it touches the scene (t in units of |d|, at most
// tmax, default unbounded), all in one call of pt_query_sweep, one JSON line each: {"sweep": [ox, oy, oz, dx, dy, dz, r], "tmax":
// <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "material": "<newmtl name>", "point": [x, y, z], "u": ..., "v": ...} (the
// contact point on the triangle and the weights of its second and third vertex there), {"sweep": [...], "tmax": ..., "hit": false} if
// nothing is touched.  A value that is not finite (tmax may be inf), a negative radius or a negative tmax is refused with exit
// status 2.
struct SweepArg { float v[8]; };
static std::vector<SweepArg> g_sweeps;
static bool parseSweep(const char* text)
{
    SweepArg w = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, INFINITY}};
    const int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f", &w.v[0], &w.v[1], &w.v[2], &w.v[3], &w.v[4], &w.v[5], &w.v[6], &w.v[7]);
    bool ok = got >= 7 && w.v[6] >= 0.0f && w.v[7] >= 0.0f;
    for (int j = 0; j < 7; j++) ok = ok && std::isfinite(w.v[j]);
    if (!ok) return false;
    g_sweeps.push_back(w);
    return true;
}
static void runSweep(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<pt_sweep_hit> out = queryRecords<pt_sweep_hit>(state, "sweep", records(g_sweeps, 8).data(), 8, g_sweeps.size(), pt_query_sweep);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_sweep_hit& r = out[i];
        const float* q = g_sweeps[i].v;
        printf("{\"sweep\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
        printFiniteOrNull(q[7]);
        if (r.prim == kNone) { printf(", \"hit\": false}\n"); continue; }
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"u\": %.9g, \"v\": %.9g}\n",
               r.t, r.prim, materialName(obj, r.material).c_str(), r.cx, r.cy, r.cz, r.u, r.v);
    }
    fflush(stdout);
}

// ---- --capsule-cast x0,y0,z0,x1,y1,z1,dx,dy,dz,r[,tmax] -----------------------------------------------------------------------
// How far the capsule of radius r around the axis {p0, p1} travels along d before it touches the scene (t in units of |d|, at most
// tmax, default unbounded), all in one call of pt_query_capsule_cast, one JSON line each: {"capsule_cast": [the ten numbers], "tmax":
// <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "material": "<newmtl name>", "point": [x, y, z], "s": ..., "feature":
// <0..5>} (the contact point on the triangle, the parameter of the axis' point that touches and pt_query_segments' feature there),
// {"capsule_cast": [...], "tmax": ..., "hit": false} if nothing is touched.  The same refusals as --sweep.
struct CapsuleCastArg { float v[12]; };
static std::vector<CapsuleCastArg> g_capsuleCasts;
static bool parseCapsuleCast(const char* text)
{
    CapsuleCastArg w = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f}};
    float* v = w.v;
    const int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &v[3], &v[7]);
    bool ok = got >= 10 && v[3] >= 0.0f && v[7] >= 0.0f;
    for (int j = 0; j < 11; j++) ok = ok && (j == 7 || std::isfinite(v[j]));
    if (!ok) return false;
    g_capsuleCasts.push_back(w);
    return true;
}
static void runCapsuleCast(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<pt_capsule_cast_hit> out =
        queryRecords<pt_capsule_cast_hit>(state, "capsule-cast", records(g_capsuleCasts, 12).data(), 12, g_capsuleCasts.size(), pt_query_capsule_cast);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_capsule_cast_hit& r = out[i];
        const float* q = g_capsuleCasts[i].v;
        printf("{\"capsule_cast\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[4], q[5], q[6], q[8], q[9], q[10], q[3]);
        printFiniteOrNull(q[7]);
        if (r.prim == kNone) { printf(", \"hit\": false}\n"); continue; }
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g], \"s\": %.9g, \"feature\": %d}\n",
               r.t, r.prim, materialName(obj, r.material).c_str(), r.cx, r.cy, r.cz, r.s, (int)r.feature);
    }
    fflush(stdout);
}

// ---- --box-cast cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax] -----------------------------------------------------------------
// How far the box of centre c and half extents h, turned by the unit quaternion q, travels along d before it touches the scene (t in
// units of |d|, at most tmax, default unbounded), all in one call of pt_query_box_cast, one JSON line each: {"box_cast": [the thirteen
// numbers], "tmax": <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "material": "<newmtl name>", "feature": <0..13>,
// "normal": [x, y, z], "point": [x, y, z]} (the winning axis of the 13-axis test, 13 for a box that starts in contact; the unit normal
// from the triangle to the box and the contact point), {"box_cast": [...], "tmax": ..., "hit": false} if nothing is touched.  Refused:
// a value that is not finite, a negative half extent or tmax, a quaternion whose squared length is off 1 by more than 1e-4.
struct BoxCastArg { float v[20]; float in[13]; };      // in: the thirteen numbers as given
static std::vector<BoxCastArg> g_boxCasts;
static bool parseBoxCast(const char* text)
{
    BoxCastArg w = {};
    float* q = w.in;
    float tmax = INFINITY;
    const int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8], &q[9], &q[10], &q[11],
                           &q[12], &tmax);
    bool ok = got >= 13 && q[3] >= 0.0f && q[4] >= 0.0f && q[5] >= 0.0f && tmax >= 0.0f;
    for (int j = 0; j < 13; j++) ok = ok && std::isfinite(q[j]);
    const float qw = q[6], qx = q[7], qy = q[8], qz = q[9];
    ok = ok && std::fabs((qw * qw + qx * qx) + (qy * qy + qz * qz) - 1.0f) <= 1e-4f;
    if (!ok) return false;
    // the rotation of the unit quaternion, row-major beside the centre: a pt_query_overlap_oriented record, then {d, tmax}
    const float m[12] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qz * qw), 2.0f * (qx * qz + qy * qw), q[0],
                         2.0f * (qx * qy + qz * qw), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qx * qw), q[1],
                         2.0f * (qx * qz - qy * qw), 2.0f * (qy * qz + qx * qw), 1.0f - 2.0f * (qx * qx + qy * qy), q[2]};
    for (int j = 0; j < 12; j++) w.v[j] = m[j];
    w.v[12] = q[3]; w.v[13] = q[4]; w.v[14] = q[5]; w.v[15] = 0.0f;
    w.v[16] = q[10]; w.v[17] = q[11]; w.v[18] = q[12]; w.v[19] = tmax;
    g_boxCasts.push_back(w);
    return true;
}
static void runBoxCast(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<pt_box_cast_hit> out = queryRecords<pt_box_cast_hit>(state, "box-cast", records(g_boxCasts, 20).data(), 20, g_boxCasts.size(), pt_query_box_cast);
    for (size_t i = 0; i < out.size(); i++) {
        const pt_box_cast_hit& r = out[i];
        const float* q = g_boxCasts[i].in;
        printf("{\"box_cast\": [");
        for (int j = 0; j < 13; j++) printf(j ? ", %.9g" : "%.9g", q[j]);
        printf("], \"tmax\": ");
        printFiniteOrNull(g_boxCasts[i].v[19]);
        if (r.prim == kNone) { printf(", \"hit\": false}\n"); continue; }
        printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"material\": \"%s\", \"feature\": %d, \"normal\": [%.9g, %.9g, %.9g], \"point\": [%.9g, %.9g, %.9g]}\n",
               r.t, r.prim, materialName(obj, r.material).c_str(), (int)r.feature, r.nx, r.ny, r.nz, r.cx, r.cy, r.cz);
    }
    fflush(stdout);
}

// ---- --cast x0,y0,z0,x1,y1,z1,x2,y2,z2,dx,dy,dz[,tmax] and --cast-mesh mesh.obj,dx,dy,dz[,tmax] -------------------------------------
// --cast: how far the triangle of these three vertices translates along d before it first touches the scene (t in units of |d|, at
// most tmax, default unbounded), all in one call of pt_query_triangle_cast, one JSON line each: {"cast": [the twelve numbers], "tmax":
// <tmax or null>, "hit": true, "t": ..., "triangle": <index>, "feature": <0..15>, "material": "<newmtl name>", "point": [x, y, z]}, or
// {"cast": [...], "tmax": ..., "hit": false}.  A value that is not finite (tmax may be inf) or a negative tmax is refused with exit
// status 2.
// --cast-mesh: the same for a whole second OBJ, as it is, by pt_set_query_mesh and pt_query_poses_cast, one JSON line each:
// {"cast_mesh": "<path>", "triangles": T, "motion": [dx, dy, dz], "tmax": ..., "hit": true, "t": ..., "triangle": <scene triangle>,
// "feature": .., "query_triangle": <the mesh triangle that touches first>, "material": .., "point": [..]}.  Text behind the last
// number is refused too.
struct CastArg { float v[16]; };
struct CastMesh { std::string path; float d[3]; float tmax; };
static std::vector<CastArg> g_casts;
static std::vector<CastMesh> g_castMeshes;
static bool parseCast(const char* text)
{
    CastArg w = {{0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    float* v = w.v;
    const int got = sscanf(text, "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[4], &v[5], &v[6], &v[8], &v[9], &v[10], &v[12], &v[13], &v[14], &v[3]);
    bool ok = got >= 12 && v[3] >= 0.0f;
    for (int j = 0; j < 15; j++) ok = ok && (j == 3 || std::isfinite(v[j]));
    if (!ok) return false;
    g_casts.push_back(w);
    return true;
}
static bool parseCastMesh(const char* value)
{
    CastMesh cm = {std::string(), {0.0f, 0.0f, 0.0f}, INFINITY};
    const std::string text = value;
    const size_t comma = text.find(',');
    cm.path = text.substr(0, comma);
    bool fine = !cm.path.empty() && comma != std::string::npos;
    if (fine) {
        int used = 0;
        const char* rest = text.c_str() + comma;
        fine = sscanf(rest, ",%f,%f,%f%n", &cm.d[0], &cm.d[1], &cm.d[2], &used) == 3;
        if (fine && rest[used] != '\0') {               // a fourth number, tmax, and nothing behind it
            int more = 0;
            fine = sscanf(rest + used, ",%f%n", &cm.tmax, &more) == 1 && rest[used + more] == '\0' && cm.tmax >= 0.0f;
        }
        for (int k = 0; k < 3; k++) if (!std::isfinite(cm.d[k])) fine = false;
    }
    if (!fine) return false;
    g_castMeshes.push_back(cm);
    return true;
}
static void printCastHit(const pt_triangle_cast_hit& r, const TinyObjWrapper& obj, bool posed)
{
    if (r.prim == kNone) { printf(", \"hit\": false}\n"); return; }
    printf(", \"hit\": true, \"t\": %.9g, \"triangle\": %u, \"feature\": %d, ", r.t, r.prim, (int)r.feature);
    if (posed) printf("\"query_triangle\": %u, ", r.query_triangle);
    printf("\"material\": \"%s\", \"point\": [%.9g, %.9g, %.9g]}\n", materialName(obj, r.material).c_str(), r.cx, r.cy, r.cz);
}
static void runCast(PathTracerState& state, const TinyObjWrapper& obj)
{
    const std::vector<pt_triangle_cast_hit> out =
        queryRecords<pt_triangle_cast_hit>(state, "cast", records(g_casts, 16).data(), 16, g_casts.size(), pt_query_triangle_cast);
    for (size_t i = 0; i < out.size(); i++) {
        const float* q = g_casts[i].v;
        printf("{\"cast\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"tmax\": ", q[0], q[1], q[2], q[4], q[5], q[6], q[8], q[9], q[10],
               q[12], q[13], q[14]);
        printFiniteOrNull(q[3]);
        printCastHit(out[i], obj, false);
    }
    fflush(stdout);
}
static void runCastMesh(PathTracerState& state, const TinyObjWrapper& obj)
{
    for (const CastMesh& m : g_castMeshes) {
        size_t T = 0;
        const std::vector<float> recs = meshRecords(m.path, T);
        const float pose[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
        const float motion[4] = {m.d[0], m.d[1], m.d[2], m.tmax};
        pt_triangle_cast_hit r;
        if (T == 0) throw Exception("cast-mesh: the mesh has no triangles");
        ptRequire(state.context, pt_set_query_mesh(state.context, recs.data(), T), "cast-mesh");
        DeviceBuffer d_pose(state.context, 48, "cast-mesh"), d_motion(state.context, 16, "cast-mesh"), d_out(state.context, sizeof(r), "cast-mesh");
        d_pose.upload(pose, 48);
        d_motion.upload(motion, 16);
        ptRequire(state.context, pt_query_poses_cast(state.context, d_pose.as<float>(), d_motion.as<float>(), 1, d_out.as<pt_triangle_cast_hit>()), "cast-mesh");
        d_out.download(&r, sizeof(r));
        printf("{\"cast_mesh\": \"%s\", \"triangles\": %zu, \"motion\": [%.9g, %.9g, %.9g], \"tmax\": ", jsonEscaped(m.path).c_str(), T, m.d[0], m.d[1], m.d[2]);
        printFiniteOrNull(m.tmax);
        printCastHit(r, obj, true);
    }
    fflush(stdout);
}

// ---- the table, in the order the options run --------------------------------------------------------------------------------
std::vector<QueryCommand>& queryCommands()
{
    static std::vector<QueryCommand> table = {
        {"--pick", "--pick x,y", parsePick, checkPick, runPick, 0},
        {"--pick-all", "--pick-all x,y[,k] with k = 1..8", parsePickAll, checkPickAll, runPickAll, 0},
        {"--nearest", "--nearest x,y,z[,radius]: finite coordinates, a radius >= 0", parseNearest, nullptr, runNearest, 0},
        {"--nearest-k", "--nearest-k x,y,z,k[,radius]: finite coordinates, k = 1..8, a radius >= 0", parseNearestK, nullptr, runNearestK, 0},
        {"--within", "--within x,y,z,radius: finite coordinates, a radius >= 0", parseWithin, nullptr, runWithin, 0},
        {"--winding", "--winding x,y,z[,beta]: finite coordinates, a beta >= 1 (inf: the exact sum)", parseWinding, nullptr, runWinding, 0},
        {"--clearance", "--clearance x0,y0,z0,x1,y1,z1[,radius]: finite coordinates, a finite radius >= 0", parseClearance, nullptr, runClearance, 0},
        {"--tri-distance", "--tri-distance x0,y0,z0,x1,y1,z1,x2,y2,z2[,radius]: nine finite coordinates, a radius >= 0", parseTriDistance, nullptr, runTriDistance, 0},
        {"--collide", "--collide mesh.obj[,tx,ty,tz[,radius]]: a file, a finite translation, a radius >= 0", parseCollide, nullptr, runCollide, 0},
        {"--overlap", "--overlap cx,cy,cz,hx,hy,hz[,k]: finite values, half extents >= 0, k = 0..8 or all", parseOverlap, nullptr, runOverlap, 0},
        {"--overlap-oriented", "--overlap-oriented cx,cy,cz,hx,hy,hz,qw,qx,qy,qz[,k]: finite values, half extents >= 0, a quaternion that is not zero, k = 0..8 or all",
         parseOverlapOriented, nullptr, runOverlapOriented, 0},
        {"--intersect", "--intersect x0,y0,z0,x1,y1,z1,x2,y2,z2[,k]: finite coordinates, k = 0..8 or all", parseIntersect, nullptr, runIntersect, 0},
        {"--sweep", "--sweep ox,oy,oz,dx,dy,dz,r[,tmax]: finite values, a radius >= 0, a tmax >= 0", parseSweep, nullptr, runSweep, 0},
        {"--capsule-cast", "--capsule-cast x0,y0,z0,x1,y1,z1,dx,dy,dz,r[,tmax]: finite values, a radius >= 0, a tmax >= 0", parseCapsuleCast, nullptr, runCapsuleCast, 0},
        {"--box-cast", "--box-cast cx,cy,cz,hx,hy,hz,qw,qx,qy,qz,dx,dy,dz[,tmax]: finite values, half extents >= 0, a unit quaternion, a tmax >= 0", parseBoxCast, nullptr,
         runBoxCast, 0},
        {"--cast", "--cast x0,y0,z0,x1,y1,z1,x2,y2,z2,dx,dy,dz[,tmax]: finite values, a tmax >= 0", parseCast, nullptr, runCast, 0},
        {"--cast-mesh", "--cast-mesh mesh.obj,dx,dy,dz[,tmax]: a file, a finite motion, a tmax >= 0", parseCastMesh, nullptr, runCastMesh, 0},
    };
    return table;
}

QueryCommand* findQueryCommand(const std::string& option)
{
    for (QueryCommand& c : queryCommands()) if (option == c.option) return &c;
    return nullptr;
}
