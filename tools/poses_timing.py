#!/usr/bin/env python3
"""Times the posed-mesh queries (pt_query_poses_any, pt_query_poses_distance) on the Cornell box beside the host path they replace and
prints ONE JSON line (also written to --out, default profiles/poses_timing.json).

One process; per figure a warm-up call, then the median of --repeats calls, each timed by the host clock around a call that returns
synchronised, with the smallest and the largest beside it: [median, min, max] in ms.

    meshes     a 12-triangle box and a tessellated sphere of 1 000 triangles, both generated here, 30 units in half extent
    pose sets  free (rotations, translations at least 60 units from everything), colliding (the centre within 20 units of the floor),
               mixed (the two interleaved); fixed seeds
    sizes      P = 4 096 and P = 262 144 poses
    new calls  through pt_debug_query_poses, which takes the flags: lanes dealt pose-major or triangle-major, each with the early look
               and the shrinking radius on (triangle-major with it is the product: pt_query_poses_any / pt_query_poses_distance) and off
               (flag bit 0, the control).  The four give the same bits, which is asserted.  The distance query runs with --radius.
    records    pt_pose_triangles, and the existing pt_query_triangles_any / pt_query_triangle_distance on the records it wrote: the
               per-triangle kernels on the same posed triangles
    parent     meshCollisions(..., pairs=False) and meshClearance(...) on the same poses as device tensors: the path before these
               calls, unchanged.  Above --parent-few posed triangles it is timed with 2 repeats instead of --repeats (stated in the
               entry); a failure to allocate is recorded as such, not hidden.
    memory     peak bytes of torch's allocator during one call of each path (the parent path allocates everything there), plus, for
               the new calls, the context's own mesh and scratch

    python tools/poses_timing.py [--sizes 4096,262144] [--repeats 20] [--radius 50] [--out profiles/poses_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_mesh(h=30.0):
    import numpy as np
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    quads = [(0, 1, 5, 4), (0, 2, 3, 1), (2, 6, 7, 3), (4, 5, 7, 6), (0, 4, 6, 2), (1, 3, 7, 5)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)


def sphere_mesh(nlon=25, nlat=21, radius=30.0):
    """2 * nlon * (nlat - 1) = 1 000 triangles"""
    import numpy as np
    v = [[0.0, -radius, 0.0]]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        v += [[radius * np.sin(th) * np.cos(2 * np.pi * j / nlon), -radius * np.cos(th), radius * np.sin(th) * np.sin(2 * np.pi * j / nlon)] for j in range(nlon)]
    v.append([0.0, radius, 0.0])
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon
    idx = [(0, ring(1, j + 1), ring(1, j)) for j in range(nlon)]
    for i in range(1, nlat - 1):
        for j in range(nlon):
            idx += [(ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i + 1, j))]
    idx += [(len(v) - 1, ring(nlat - 1, j), ring(nlat - 1, j + 1)) for j in range(nlon)]
    return np.array(v, np.float32), np.array(idx, np.int64)


def pose_set(name, n, seed):
    """(n, 3, 4) float32: rotations about random axes; free translations in the open part of the Cornell box (60 units from the walls,
    the blocks and the small objects), colliding ones over open floor with the centre at most 20 units above it"""
    import numpy as np
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    m = np.zeros((n, 3, 4))
    m[:, 0, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1)
    m[:, 1, :3] = np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1)
    m[:, 2, :3] = np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    free = rng.uniform([70.0, 180.0, 340.0], [190.0, 400.0, 480.0], (n, 3))
    low = rng.uniform([70.0, 0.0, 340.0], [190.0, 20.0, 480.0], (n, 3))
    m[:, :, 3] = {"free": free, "colliding": low, "mixed": np.where((np.arange(n) % 2 == 0)[:, None], free, low)}[name]
    return m.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,262144")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--parent-few", type=int, default=1 << 26, help="posed triangles above which the parent path gets 2 repeats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poses_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    L = _native.hip()
    if not torch.cuda.is_available():
        raise SystemExit("poses_timing: no GPU (a timing from anywhere else says nothing)")
    out = {"tool": "poses_timing", "repeats": a.repeats, "radius": a.radius, "figures": "[median, min, max] ms", "kernel_source_hash": L.pt_kernel_source_hash().decode(),
           "device": torch.cuda.get_device_name(0), "runs": []}
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    dev = torch.device("cuda", state._device)

    def timed(fn, repeats):
        fn()                                        # warm-up: code object load, first-use allocations
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)]

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        got = fn()
        torch.cuda.synchronize()
        return got, int(torch.cuda.max_memory_allocated(dev) - base)

    def check(rc):
        assert rc == 0, L.pt_last_error(state.context)

    try:
        for mesh_name, (v, idx) in (("box12", box_mesh()), ("sphere1000", sphere_mesh())):
            T = pt.setQueryMesh(state, v, idx)
            tv, ti = torch.as_tensor(v, device=dev), torch.as_tensor(idx, device=dev)
            for size in a.sizes.split(","):
                P = int(size)
                for k, set_name in enumerate(("free", "mixed", "colliding")):
                    poses = torch.as_tensor(pose_set(set_name, P, 100 + k), device=dev)
                    flat = poses.view(P, 12)
                    hit = torch.empty((P,), dtype=torch.uint8, device=dev)
                    rec = torch.empty((P, 12), dtype=torch.float32, device=dev)
                    torch.cuda.synchronize()
                    run = {"mesh": mesh_name, "triangles": T, "poses": P, "set": set_name, "posed_triangles": P * T}
                    ms, answers = {}, {}
                    for order, obit in (("triangle_major", 0), ("pose_major", _native.POSES_POSE_MAJOR)):
                        for early, ebit in (("early", 0), ("no_early", _native.POSES_NO_EARLY)):
                            flags = obit | ebit
                            ms["any_%s_%s" % (order, early)] = timed(lambda: check(L.pt_debug_query_poses(state.context, flat.data_ptr(), P, 0.0, hit.data_ptr(), None, None, flags)), a.repeats)
                            ms["distance_%s_%s" % (order, early)] = timed(lambda: check(L.pt_debug_query_poses(state.context, flat.data_ptr(), P, a.radius, None, None, rec.data_ptr(), flags)), a.repeats)
                            got = (hit.clone(), rec.view(torch.int32).clone())
                            if answers:
                                assert torch.equal(got[0], answers["hit"]) and torch.equal(got[1], answers["rec"]), "the flags changed an answer"
                            answers = {"hit": got[0], "rec": got[1]}
                    _, mem_any = peak(lambda: pt.queryPosesAny(state, poses))
                    _, mem_dist = peak(lambda: pt.queryPosesDistance(state, poses, max_radius=a.radius))
                    own = pt.getQueryMesh(state)["device_bytes"] + 8 * P
                    run["new_peak_bytes"] = {"any": mem_any + own, "distance": mem_dist + own, "of_which_mesh_and_scratch": own}
                    run["hit_share"] = round(float(answers["hit"].float().mean()), 4)
                    run["found_share"] = round(float((answers["rec"][:, 1] != -1).float().mean()), 4)
                    # the per-triangle kernels on the materialised records
                    try:
                        posed = torch.empty((P * T, 12), dtype=torch.float32, device=dev)
                        per = torch.empty((P * T,), dtype=torch.uint8, device=dev)
                        torch.cuda.synchronize()
                        ms["pose_triangles"] = timed(lambda: check(L.pt_pose_triangles(state.context, flat.data_ptr(), P, posed.data_ptr())), a.repeats)
                        ms["triangles_any_on_records"] = timed(lambda: check(L.pt_query_triangles_any(state.context, posed.data_ptr(), P * T, per.data_ptr())), a.repeats)
                        assert torch.equal(per.view(P, T).any(1), answers["hit"] != 0), "pt_query_triangles_any on the records disagrees"
                        del posed, per
                    except torch.cuda.OutOfMemoryError as e:
                        run["records_failed"] = "out of memory: %s" % str(e).splitlines()[0]
                    # the parent's path
                    few = 2 if P * T > a.parent_few else a.repeats
                    run["parent_repeats"] = few
                    try:
                        ms["parent_meshCollisions"] = timed(lambda: pt.meshCollisions(state, tv, ti, poses), few)
                        old_hit, mem = peak(lambda: pt.meshCollisions(state, tv, ti, poses))
                        run["parent_peak_bytes"] = {"meshCollisions": mem}
                        run["parent_hit_agrees_share"] = round(float((old_hit == (answers["hit"] != 0)).float().mean()), 6)
                        del old_hit
                        ms["parent_meshClearance"] = timed(lambda: pt.meshClearance(state, tv, ti, poses, max_radius=a.radius), few)
                        old, mem = peak(lambda: pt.meshClearance(state, tv, ti, poses, max_radius=a.radius))
                        run["parent_peak_bytes"]["meshClearance"] = mem
                        run["parent_found_agrees_share"] = round(float((torch.isfinite(old["clearance"]) == (answers["rec"][:, 1] != -1)).float().mean()), 6)
                        del old
                    except torch.cuda.OutOfMemoryError as e:
                        run["parent_failed"] = "out of memory: %s" % str(e).splitlines()[0]
                    torch.cuda.empty_cache()
                    run["ms"] = ms
                    out["runs"].append(run)
                    print("poses_timing: %s P=%d %s done" % (mesh_name, P, set_name), file=sys.stderr, flush=True)
    finally:
        pt.CleanAllTheThings(state)
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
