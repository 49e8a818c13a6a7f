#!/usr/bin/env python3
"""Times the translating-triangle casts (pt_query_triangle_cast, pt_query_triangle_cast_any, pt_query_poses_cast) on the Cornell box and
prints ONE JSON line (also written to --out, default profiles/tricast_timing.json).

Every figure is the host wall time of a call that returns synchronised: one process, a warm-up call, [median, min, max] ms of --repeats —
but the advancement loop, a sequence of 60 to 70 calls, whose figure is [median, min, max] of --advance-repeats whole runs after one
warm-up run (the JSON says so beside it).

Per-triangle, n triangles of --size of the scene box's diagonal, centres uniform in the box, random motions of up to one diagonal:
    cast, cast_any                 the two calls; from the counting twin (not timed) the mean and maximum inner nodes visited and
                                   triangles tested per cast
    cast_large                     the same casts with triangles five times the size: what a large diagonal query costs in visits
    triangle_distance              pt_query_triangle_distance on the same triangles, no limit on the distance
    sweep_r0                       pt_query_sweep with radius 0 from their centroids along the same motions
Posed, P poses of poses_timing.py's 1 000-triangle sphere (its "free" and "mixed" sets) moving by up to 300 units towards the floor:
    poses_cast                     pt_query_poses_cast
    materialised                   the route without it (meshCast's, on the device): pt_pose_triangles, pt_query_triangle_cast on the
                                   P x T casts, the reduction per pose; at most --materialise-poses poses
    advancement                    what a caller runs today, on --advance-poses poses: pt_query_poses_distance, step every pose by its
                                   clearance, again, until every pose is within --bound of the scene or at tmax; calls and ms

    python tools/tricast_timing.py [--n 2000000] [--poses 4096,262144] [--repeats 30] [--out profiles/tricast_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--size", type=float, default=0.02)
    ap.add_argument("--poses", default="4096,262144")
    ap.add_argument("--materialise-poses", type=int, default=16384)
    ap.add_argument("--advance-poses", type=int, default=4096)
    ap.add_argument("--bound", type=float, default=3e-4, help="the host test's contact bound: where the advancement loop stops")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--advance-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tricast_timing.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import acgpathtracing_amd as pt
    from acgpathtracing_amd import _native
    import poses_timing
    L = _native.hip()
    if not torch.cuda.is_available():
        raise SystemExit("tricast_timing: no GPU (a timing from anywhere else says nothing)")
    state, _ = pt.setup(os.path.join(pt.SCENES, "cornell_box.obj"), width=64, height=64, max_depth=4, spp=1)
    dev = torch.device("cuda", state._device)
    info = pt.getBvhInfo(state)
    lo, hi = np.array([float(x) for x in info.scene_lo]), np.array([float(x) for x in info.scene_hi])
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    out = {"tool": "tricast_timing", "repeats": a.repeats, "figures": "[median, min, max] ms of `repeats` calls after a warm-up call; the advancement loops: see their own `figures`", "kernel_source_hash": L.pt_kernel_source_hash().decode(),
           "device": torch.cuda.get_device_name(0), "triangles": int(info.n_tris), "diagonal": diag}

    def timed(fn, repeats=None):
        fn()                                        # warm-up: code object load, first-use allocations
        ts = []
        for _ in range(repeats or a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)]

    def visits_of(casts):
        n = casts.shape[0]
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        vis = torch.empty((n, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.pt_debug_triangle_cast_visits(state.context, casts.data_ptr(), n, rec.data_ptr(), vis.data_ptr()) == 0, L.pt_last_error(state.context)
        v = vis.cpu().numpy().astype(np.int64)
        return {"nodes_mean": round(float(v[:, 0].mean()), 2), "triangles_mean": round(float(v[:, 1].mean()), 2), "nodes_max": int(v[:, 0].max()),
                "triangles_max": int(v[:, 1].max()), "hit_share": round(float((rec[:, 0] >= 0).float().mean()), 4),
                "start_overlap_share": round(float((rec[:, 0] == 0).float().mean()), 4)}

    try:
        # ---- per triangle ----
        n = a.n
        rng = np.random.default_rng(3737)
        centre = lo + rng.random((n, 3)) * (hi - lo)

        def shapes(size):
            off = rng.normal(size=(n, 3, 3))
            off -= off.mean(axis=1, keepdims=True)
            off /= np.sqrt((off * off).sum(axis=2)).max(axis=1)[:, None, None]
            return centre[:, None, :] + off * (size * diag)
        u = rng.normal(size=(n, 3))
        u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
        d = u * (diag * rng.uniform(0.05, 1.0, (n, 1)))
        per = {}
        for name, size in (("small", a.size), ("large", 5 * a.size)):
            tri = shapes(size)
            casts = np.zeros((n, 16), np.float32)
            casts[:, 0:3], casts[:, 4:7], casts[:, 8:11], casts[:, 12:15], casts[:, 3] = tri[:, 0], tri[:, 1], tri[:, 2], d, 1.0
            x = torch.from_numpy(casts).to(dev)
            ms = {"cast": timed(lambda: pt.queryTriangleCast(state, x))}
            if name == "small":
                ms["cast_any"] = timed(lambda: pt.queryTriangleCast(state, x, any_hit=True))
                recs = x[:, 0:12].clone()
                recs[:, 3] = float("inf")
                ms["triangle_distance"] = timed(lambda: pt.queryTriangleDistance(state, recs))
                sweeps = np.zeros((n, 8), np.float32)
                sweeps[:, 0:3], sweeps[:, 3:6], sweeps[:, 7] = tri.mean(axis=1), d, 1.0
                sw = torch.from_numpy(sweeps).to(dev)
                ms["sweep_r0"] = timed(lambda: pt.querySweep(state, sw))
                del recs, sw
            per[name] = {"size_of_diagonal": size, "ms": ms, "mcasts_per_s": round(n / ms["cast"][0] / 1e3, 1), "visits": visits_of(x)}
            del x
        per["small"]["cast_over_triangle_distance"] = round(per["small"]["ms"]["cast"][0] / per["small"]["ms"]["triangle_distance"][0], 3)
        per["small"]["cast_over_sweep_r0"] = round(per["small"]["ms"]["cast"][0] / per["small"]["ms"]["sweep_r0"][0], 3)
        per["large_over_small_nodes"] = round(per["large"]["visits"]["nodes_mean"] / per["small"]["visits"]["nodes_mean"], 3)
        out["per_triangle"] = {"casts": n, **per}

        # ---- posed ----
        v, idx = poses_timing.sphere_mesh()
        T = pt.setQueryMesh(state, v, idx)
        runs = []
        for size in a.poses.split(","):
            P = int(size)
            for k, set_name in enumerate(("free", "mixed")):
                poses = torch.as_tensor(poses_timing.pose_set(set_name, P, 300 + k), device=dev).view(P, 12).contiguous()
                mrng = np.random.default_rng(400 + k)
                motions = np.zeros((P, 4), np.float32)
                motions[:, 0:3] = np.stack([mrng.uniform(-100, 100, P), mrng.uniform(-300, -50, P), mrng.uniform(-100, 100, P)], axis=1)
                motions[:, 3] = 1.0
                tm = torch.from_numpy(motions).to(dev)
                run = {"poses": P, "set": set_name, "mesh_triangles": T, "ms": {"poses_cast": timed(lambda: pt.queryPosesCast(state, poses, tm))}}
                got = pt.queryPosesCast(state, poses, tm)
                run["hit_share"] = round(float((got["t"] >= 0).float().mean()), 4)
                run["start_overlap_share"] = round(float((got["t"] == 0).float().mean()), 4)
                Pm = min(P, a.materialise_poses)

                def materialised():
                    posed = pt.posedTriangles(state, poses[:Pm])
                    casts = torch.zeros((Pm, T, 16), dtype=torch.float32, device=dev)
                    casts[:, :, 0:12] = posed
                    casts[:, :, 3] = tm[:Pm, None, 3]
                    casts[:, :, 12:15] = tm[:Pm, None, 0:3]
                    t = pt.queryTriangleCast(state, casts.view(Pm * T, 16))["t"].view(Pm, T)
                    return torch.where(t >= 0, t, torch.full_like(t, float("inf"))).min(dim=1).values
                run["materialised_poses"] = Pm
                run["ms"]["materialised"] = timed(materialised)
                run["ms"]["poses_cast_same_poses"] = timed(lambda: pt.queryPosesCast(state, poses[:Pm].contiguous(), tm[:Pm].contiguous()))
                best = materialised()
                same = pt.queryPosesCast(state, poses[:Pm].contiguous(), tm[:Pm].contiguous())["t"]
                assert torch.equal(torch.where(same >= 0, same, torch.full_like(same, float("inf"))), best)
                # conservative advancement by hand
                Pa = min(P, a.advance_poses)
                base, mo = poses[:Pa].clone().view(Pa, 3, 4), tm[:Pa]
                speed = torch.sqrt((mo[:, 0:3] ** 2).sum(dim=1))
                loop = {}

                def advance():
                    t_now = torch.zeros(Pa, device=dev)
                    done = torch.zeros(Pa, dtype=torch.bool, device=dev)
                    calls = 0
                    while calls < 200 and not bool(done.all()):
                        cur = base.clone()
                        cur[:, :, 3] += mo[:, 0:3] * t_now[:, None]
                        clear = pt.queryPosesDistance(state, cur.view(Pa, 12))["clearance"]
                        calls += 1
                        done |= (clear <= a.bound) | (t_now >= mo[:, 3])
                        t_now = torch.where(done, t_now, torch.minimum(t_now + clear / speed, mo[:, 3]))
                    loop["calls"], loop["finished"] = calls, round(float(done.float().mean()), 4)
                adv_ms = timed(advance, a.advance_repeats)
                run["advancement"] = {"poses": Pa, "calls": loop["calls"], "ms": adv_ms, "figures": "[median, min, max] ms of %d whole runs after a warm-up run" % a.advance_repeats,
                                      "finished_share": loop["finished"],
                                      "poses_cast_ms_same_poses": timed(lambda: pt.queryPosesCast(state, poses[:Pa].contiguous(), tm[:Pa].contiguous()))[0]}
                runs.append(run)
                del poses, tm
        out["posed"] = runs
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
