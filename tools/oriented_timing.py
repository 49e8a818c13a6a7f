#!/usr/bin/env python3
"""Times the oriented-box overlap queries (pt_query_overlap_oriented, _any, _lists, pt_pose_boxes) on the Cornell box beside the calls a
caller had before them and prints ONE JSON line (also written to --out, default profiles/oriented_timing.json).

overlap_timing.py's method: one process; per figure a warm-up call, then the median of --repeats calls, each timed by the host clock
around a call that returns synchronised, with the smallest and the largest beside it: [median, min, max] in ms.

    grid_frame   an occupancy grid of --boxes cells over the scene box, turned by one rotation about the scene's centre, through the
                 oriented calls; beside it pt_query_overlap on the same cells unturned (the parent's kernel: the yardstick)
    identity     the unturned cells as oriented records with the exact identity, against pt_query_overlap on them: the same answers,
                 so the difference is what the nine dot products and the three box axes of the admission cost
    links        --boxes elongated boxes (one half extent 5 - 20 % of the diagonal, the others 0.2 - 2 %, uniform random rotations)
                 through the oriented calls, beside pt_query_overlap on their world AABBs; the visits of both (inner nodes and triangles
                 per box, from the counting twins), how many times the triangles the AABBs report, and the share of AABBs that report an
                 occupied box although the oriented box is empty
    lists        the complete-lists sequence on the links: the counting call, pt_list_offsets, pt_query_overlap_oriented_lists
    admission    the counting walk with the six axes of the product (pt_debug_overlap_oriented_visits) against the same walk with the nine
                 axes cross(world axis, box axis) added (pt_debug_overlap_oriented_visits_cross), on the links and on the turned grid:
                 time and visits of both
    poses        --poses poses of poses_timing.py's sphere (its free / mixed / colliding sets): pt_pose_boxes plus
                 pt_query_overlap_oriented_any on the padded bounding box (posedMeshBoxes' pad), beside pt_query_poses_any on the same
                 poses, with the share of poses the box alone clears

    python tools/oriented_timing.py [--boxes 2097152] [--poses 262144] [--repeats 30] [--out profiles/oriented_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 21)
    ap.add_argument("--poses", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import oriented_ref as ob
    from nearest_timing import grid_shape
    from poses_timing import pose_set, sphere_mesh
    L = _native.hip()
    if not torch.cuda.is_available():
        raise SystemExit("oriented_timing: no GPU (a timing from anywhere else says nothing)")
    state, obj = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    dev = torch.device("cuda", state._device)
    ctx = state.context
    out = {"tool": "oriented_timing", "repeats": a.repeats, "figures": "[median, min, max] ms", "kernel_source_hash": L.pt_kernel_source_hash().decode(),
           "device": torch.cuda.get_device_name(0), "admission_shipped": "six axes: three world, three box"}

    def check(rc):
        assert rc == 0, L.pt_last_error(ctx)

    def timed(fn):
        fn()                                        # warm-up: code object load, first-use allocations
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)]

    def up(x):
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        torch.cuda.synchronize()
        return t

    def three(prefix, call, any_call, d, n, hit, prims, counts, ms):
        ms[prefix + "_any"] = timed(lambda: check(any_call(ctx, d.data_ptr(), n, hit.data_ptr())))
        ms[prefix + "_count"] = timed(lambda: check(call(ctx, d.data_ptr(), n, 0, None, counts.data_ptr())))
        ms[prefix + "_list8"] = timed(lambda: check(call(ctx, d.data_ptr(), n, 8, prims.data_ptr(), counts.data_ptr())))

    def visits(fn, d, n, counts, vis):
        check(fn(ctx, d.data_ptr(), n, counts.data_ptr(), vis.data_ptr()))
        v, c = vis.cpu().numpy().view(np.uint32).reshape(n, 2), counts.cpu().numpy().view(np.uint32)
        return {"nodes_mean": round(float(v[:, 0].mean()), 2), "triangles_mean": round(float(v[:, 1].mean()), 2), "nodes_max": int(v[:, 0].max()),
                "triangles_max": int(v[:, 1].max()), "count_mean": round(float(c.mean()), 3), "occupied_share": round(float((c != 0).mean()), 4)}, c.copy()

    try:
        info = pt.getBvhInfo(state)
        lo, hi = np.array([float(x) for x in info.scene_lo]), np.array([float(x) for x in info.scene_hi])
        cen, diag = 0.5 * (lo + hi), float(np.sqrt(((hi - lo) ** 2).sum()))
        shape = grid_shape(a.boxes)
        n = int(np.prod(shape))
        hit = torch.empty((n,), dtype=torch.uint8, device=dev)
        prims = torch.empty((n, 8), dtype=torch.int32, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        vis = torch.empty((n, 2), dtype=torch.int32, device=dev)
        ms = {}
        # ---- the grid, turned and not
        rot = ob.rotations(np.random.default_rng(3803), 1)[0]
        frame = np.hstack([rot.astype(np.float64), (cen - rot.astype(np.float64) @ cen)[:, None]])      # a turn about the scene's centre
        cells = pt.occupancyBoxes(shape, lo, hi)
        d_cells, d_turned = up(cells), up(pt.occupancyBoxes(shape, lo, hi, frame=frame))
        d_ident = up(pt.orientedBoxes(cells[:, 0:3], cells[:, 3:6], np.eye(3)))
        three("grid_aabb", L.pt_query_overlap, L.pt_query_overlap_any, d_cells, n, hit, prims, counts, ms)
        want = counts.clone()
        three("grid_identity", L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_any, d_ident, n, hit, prims, counts, ms)
        assert torch.equal(want, counts), "the identity records answer differently from pt_query_overlap"
        three("grid_frame", L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_any, d_turned, n, hit, prims, counts, ms)
        v_aabb, _ = visits(L.pt_debug_overlap_visits, d_cells, n, counts, vis)
        v_ident, _ = visits(L.pt_debug_overlap_oriented_visits, d_ident, n, counts, vis)
        v_frame, _ = visits(L.pt_debug_overlap_oriented_visits, d_turned, n, counts, vis)
        ab = {}

        def admission(name, d):
            six, c6 = visits(L.pt_debug_overlap_oriented_visits, d, n, counts, vis)
            fifteen, c15 = visits(L.pt_debug_overlap_oriented_visits_cross, d, n, counts, vis)
            assert np.array_equal(c6, c15), "the cross axes changed a count"
            t6 = timed(lambda: check(L.pt_debug_overlap_oriented_visits(ctx, d.data_ptr(), n, counts.data_ptr(), vis.data_ptr())))
            t15 = timed(lambda: check(L.pt_debug_overlap_oriented_visits_cross(ctx, d.data_ptr(), n, counts.data_ptr(), vis.data_ptr())))
            ab[name] = {"six_axes": {"ms": t6, "nodes_mean": six["nodes_mean"], "triangles_mean": six["triangles_mean"]},
                        "fifteen_axes": {"ms": t15, "nodes_mean": fifteen["nodes_mean"], "triangles_mean": fifteen["triangles_mean"]},
                        "fifteen_over_six_ms": round(t15[0] / t6[0], 3)}

        admission("grid_frame", d_turned)
        out["grid"] = {"boxes": n, "grid": list(shape), "visits": {"aabb": v_aabb, "identity": v_ident, "frame": v_frame},
                       "identity_over_aabb_any": round(ms["grid_identity_any"][0] / ms["grid_aabb_any"][0], 3),
                       "frame_over_aabb_any": round(ms["grid_frame_any"][0] / ms["grid_aabb_any"][0], 3)}
        del d_cells, d_turned, d_ident
        # ---- the links and their world AABBs
        rng = np.random.default_rng(3802)
        c = lo + rng.random((n, 3)) * (hi - lo)
        h = diag * rng.uniform(0.002, 0.02, (n, 3))
        h[np.arange(n), rng.integers(0, 3, n)] = diag * rng.uniform(0.05, 0.20, n)
        links = pt.orientedBoxes(c.astype(np.float32), h.astype(np.float32), ob.rotations(rng, n))
        d_links, d_aabbs = up(links), up(ob.world_aabbs(links))
        three("links", L.pt_query_overlap_oriented, L.pt_query_overlap_oriented_any, d_links, n, hit, prims, counts, ms)
        three("links_aabb", L.pt_query_overlap, L.pt_query_overlap_any, d_aabbs, n, hit, prims, counts, ms)
        v_links, c_links = visits(L.pt_debug_overlap_oriented_visits, d_links, n, counts, vis)
        admission("links", d_links)
        out["admission_ab"] = ab
        v_laabb, c_aabb = visits(L.pt_debug_overlap_visits, d_aabbs, n, counts, vis)
        assert (c_aabb >= c_links).all(), "a world AABB reports fewer triangles than its box"
        out["links"] = {"boxes": n, "visits": {"oriented": v_links, "aabb": v_laabb},
                        "aabb_reports_times_the_triangles": round(float(c_aabb.sum()) / max(float(c_links.sum()), 1.0), 2),
                        "aabb_occupied_but_box_empty_share": round(float(((c_aabb != 0) & (c_links == 0)).sum()) / max(float((c_aabb != 0).sum()), 1.0), 4),
                        "oriented_over_aabb_any": round(ms["links_any"][0] / ms["links_aabb_any"][0], 3),
                        "oriented_over_aabb_count": round(ms["links_count"][0] / ms["links_aabb_count"][0], 3)}
        # ---- the complete lists of the links
        off = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
        total = C.c_uint64(0)
        check(L.pt_query_overlap_oriented(ctx, d_links.data_ptr(), n, 0, None, counts.data_ptr()))
        check(L.pt_list_offsets(ctx, counts.data_ptr(), n, off.data_ptr(), C.byref(total)))
        flat = torch.empty((max(int(total.value), 1),), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ms["links_lists_count"] = ms["links_count"]
        ms["links_lists_offsets"] = timed(lambda: check(L.pt_list_offsets(ctx, counts.data_ptr(), n, off.data_ptr(), C.byref(total))))
        ms["links_lists_fill"] = timed(lambda: check(L.pt_query_overlap_oriented_lists(ctx, d_links.data_ptr(), n, off.data_ptr(), flat.data_ptr(), int(total.value), None)))
        out["lists"] = {"boxes": n, "indices": int(total.value), "sequence_ms": round(ms["links_lists_count"][0] + ms["links_lists_offsets"][0] + ms["links_lists_fill"][0], 4)}
        del d_links, d_aabbs, off, flat, prims, vis
        # ---- posed bounding boxes beside the posed-mesh query
        v, idx = sphere_mesh()
        T = pt.setQueryMesh(state, v, idx)
        P = a.poses
        out["poses"] = {"mesh": "sphere1000", "triangles": T, "poses": P, "sets": {}}
        pad = pt.posedMeshBoxPad(v, 600.0)
        lb = pt.pathtracer._local_box("oriented_timing", v.min(axis=0).astype(np.float64) - pad, v.max(axis=0).astype(np.float64) + pad)
        p_lb = lb.ctypes.data_as(C.POINTER(C.c_float))
        recs = torch.empty((P, 16), dtype=torch.float32, device=dev)
        bhit, phit = torch.empty((P,), dtype=torch.uint8, device=dev), torch.empty((P,), dtype=torch.uint8, device=dev)
        for k, set_name in enumerate(("free", "mixed", "colliding")):
            poses = up(pose_set(set_name, P, 100 + k).reshape(P, 12))
            pm = {"pose_boxes": timed(lambda: check(L.pt_pose_boxes(ctx, poses.data_ptr(), P, p_lb, recs.data_ptr()))),
                  "boxes_any": timed(lambda: check(L.pt_query_overlap_oriented_any(ctx, recs.data_ptr(), P, bhit.data_ptr()))),
                  "poses_any": timed(lambda: check(L.pt_query_poses_any(ctx, poses.data_ptr(), P, phit.data_ptr(), None)))}
            assert not ((bhit == 0) & (phit != 0)).any(), "a pose whose padded box is free collides"
            out["poses"]["sets"][set_name] = {"ms": pm, "box_clears_share": round(float((bhit == 0).float().mean()), 4), "collide_share": round(float((phit != 0).float().mean()), 4)}
        out["ms"] = ms
        out["mboxes_per_s"] = {k: round(n / t[0] / 1e3, 1) for k, t in ms.items() if not k.startswith("links_lists")}
    finally:
        pt.CleanAllTheThings(state)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
