"""The calibration of pt_firefly_filter's defaults, on the CPU oracle and the NumPy references only.

The oracle's Cornell box (glass and metal) at 128 x 128, maxDepth 8, direct lighting and importance sampling; the input is one 8-spp
launch, repeated with the frame indices 0 .. 7 (8 disjoint seed sets); the truth is tests/golden/denoise_cornell_128.npz (8192 spp).
For every (ratio, rank, radius) of the grid it prints the MSE of the noisy, the filtered, the denoised and the
filtered-then-denoised image (mean and sample standard deviation over the 8 inputs), what the filter costs the converged image and
the energy it removes from it.  `--twin` repeats the sweep on light mode 1 with the microfacet model, against a truth rendered here.

    python tools/firefly_sweep.py [--twin] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import acgpathtracing_amd as pt                                    # noqa: E402
from acgpathtracing_amd import _build                              # noqa: E402
import denoise_ref as dr                                           # noqa: E402
import firefly_ref as fr                                           # noqa: E402
import oracle_lib                                                  # noqa: E402
from scene_utils import copy_params, image_mse, make_params       # noqa: E402

RATIOS, RANKS, RADII, RUNS = (1.5, 2, 3, 4, 6, 8, 16), (1, 2, 3), (1, 2), 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--twin", action="store_true", help="light mode 1, microfacet materials; the truth is rendered here (1024 spp)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    _build.build_host(); _build.build_oracle()
    orc = oracle_lib.load()
    obj = pt.TinyObjWrapper(os.path.join(pt.SCENES, "cornell_box.obj"))
    sc = orc.scene(obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), obj.getMaterials())
    gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_cornell_128.npz"))
    size, _, depth, _, _ = (int(v) for v in gold["meta"])
    one = np.ones((size, size, 1), np.float32)
    if a.twin:
        sc.set_light_mode(1); sc.set_material_model(1)
        acc = np.zeros((size, size, 4), np.float64)
        for f in range(16):       # 16 frames of 64 spp, indices past the inputs'
            fa, _, _, _ = sc.render(copy_params(make_params(size, size, 64, depth, True, True, frame=100 + f)))
            acc += fa.astype(np.float64) * (101 + f)
        ref = np.concatenate([(acc[..., :3] / 16).astype(np.float32), one], axis=-1)
    else:
        ref = np.concatenate([gold["ref"], one], axis=-1)
    p = make_params(size, size, 8, depth, True, True)
    rays = dr.pixel_rays(size, size, p.cameraEye.tuple(), p.cameraU.tuple(), p.cameraV.tuple(), p.cameraW.tuple())
    t, prim = sc.trace_closest(rays, use_bvh=True)
    diffuse = np.array([[m.diffuse.x, m.diffuse.y, m.diffuse.z] for m in obj.getMaterials()], np.float32)
    alb, nd = dr.features_from_hits(rays, t, prim, obj.getVerticesFloat(), obj.getIndexBuffer(), obj.getMaterialIndices(), diffuse)
    alb, nd = alb.reshape(size, size, 4), nd.reshape(size, size, 4)

    noisy = []
    for r in range(RUNS):
        # a launch with frame index r onto a zero accumulation leaves frame / (r + 1)
        acc, _, _, _ = sc.render(copy_params(make_params(size, size, 8, depth, True, True, frame=r)))
        acc = acc.reshape(size, size, 4).copy(); acc[..., :3] *= np.float32(r + 1); acc[..., 3] = 1
        noisy.append(acc)
    m_noisy = np.array([image_mse(x, ref) for x in noisy])
    m_dn = np.array([image_mse(dr.denoise(x, alb, nd, 5), ref) for x in noisy])
    m_edge = image_mse(dr.denoise(ref, alb, nd, 5), ref)
    print("noisy    %.4e +- %.2e   %s" % (m_noisy.mean(), m_noisy.std(ddof=1), " ".join("%.3e" % v for v in m_noisy)))
    print("denoised %.4e +- %.2e   %s" % (m_dn.mean(), m_dn.std(ddof=1), " ".join("%.3e" % v for v in m_dn)))
    print("denoise(ref) costs %.4e = %.4f of the noisy MSE" % (m_edge, m_edge / m_noisy.mean()))
    rows = []
    print("ratio rank radius | filtered  | filt+denoised +- sd | gain G = dn / fdn: mean +- sd (min .. max) | cost(ref)/noisy removed(ref) | clamped@8spp")
    for radius in RADII:
        for rank in RANKS:
            for ratio in RATIOS:
                kw = dict(ratio=ratio, rank=rank, radius=radius, floor=0.01)
                filt = [fr.filter(x, **kw) for x in noisy]
                m_f = np.array([image_mse(o, ref) for o, _ in filt])
                m_fd = np.array([image_mse(dr.denoise(o, alb, nd, 5), ref) for o, _ in filt])
                gain = m_dn / m_fd
                fo, fi = fr.filter(ref, **kw)
                cost = image_mse(fo, ref) / m_noisy.mean()
                row = dict(ratio=ratio, rank=rank, radius=radius, filtered=float(m_f.mean()), fdn=float(m_fd.mean()), fdn_sd=float(m_fd.std(ddof=1)),
                           gain=float(gain.mean()), gain_sd=float(gain.std(ddof=1)), gain_min=float(gain.min()), gain_max=float(gain.max()),
                           gains=[float(g) for g in gain], cost=float(cost), removed=fr.removed_share(fi),
                           clamped=float(np.mean([i["clamped_pixels"] for _, i in filt])))
                rows.append(row)
                print("%5.1f %4d %6d | %.3e | %.3e +- %.1e | %.3f +- %.3f (%.3f .. %.3f) | %.4f %.4f | %.0f" % (
                    ratio, rank, radius, row["filtered"], row["fdn"], row["fdn_sd"], row["gain"], row["gain_sd"], row["gain_min"], row["gain_max"],
                    row["cost"], row["removed"], row["clamped"]), flush=True)
    limit = m_edge / m_noisy.mean()
    allowed = [r for r in rows if r["cost"] < limit]
    best = min(allowed, key=lambda r: r["fdn"]) if allowed else None
    print("cost limit %.4f; the best allowed setting: %s" % (limit, best))
    if a.json:
        json.dump({"noisy": m_noisy.tolist(), "denoised": m_dn.tolist(), "edge": m_edge, "rows": rows, "best": best}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
