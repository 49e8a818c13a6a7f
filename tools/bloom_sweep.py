"""The table behind pt_bloom's default intensity, on the NumPy references only.

The image is the truth of the CPU oracle's Cornell box at 128 x 128 (tests/golden/denoise_cornell_128.npz, 8192 spp), exposed as
tests/display_ref.py meters it with the display transform's defaults.  threshold 1, knee 0.5 and clamp 0 are display units and are
divided by that exposure in fp32, as displayTransform(bloom=) does; spread 1, levels 6.  For every intensity it prints the bright
share of the luminance (what went into the pyramid) and by how much the glare raises the image's mean luminance; the default is the
largest intensity of the list whose increase stays below 2 %.

    python tools/bloom_sweep.py [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bloom_ref as br                                             # noqa: E402
import display_ref as dr                                           # noqa: E402

INTENSITIES = (0.02, 0.05, 0.1, 0.2, 0.5)
LIMIT = 0.02
F = np.float32


def table(img, exposure, intensities=INTENSITIES):
    """rows of (intensity, bright_share, relative increase of the mean luminance) for a float32 [h, w, 4] image"""
    e = F(exposure)
    base = br.params()
    scaled = dict(threshold=F(base["threshold"]) / e, knee=F(base["knee"]) / e, clamp=F(base["clamp"]) / e)
    mean0 = float(np.mean(br.lum(img[..., :3]).astype(np.float64)))
    rows = []
    for intensity in intensities:
        out, info, _ = br.bloom(img, dict(scaled, intensity=intensity))
        mean1 = float(np.mean(br.lum(out[..., :3]).astype(np.float64)))
        rows.append(dict(intensity=intensity, bright_share=br.bright_share(info), bright_pixels=info["bright_pixels"], increase=mean1 / mean0 - 1.0))
    return rows


def pick(rows, limit=LIMIT):
    ok = [r["intensity"] for r in rows if r["increase"] < limit]
    return max(ok) if ok else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_cornell_128.npz"))
    ref = np.asarray(gold["ref"], F)
    img = np.concatenate([ref, np.ones(ref.shape[:2] + (1,), F)], axis=-1)
    exposure = dr.transform(img.reshape(-1, 4), dr.params())[1]["exposure"]
    rows = table(img, exposure)
    print("metered exposure %.6g: threshold %.6g, knee %.6g in radiance units; levels built %d" % (
        exposure, 1.0 / exposure, 0.5 / exposure, len(br.levels_of(img.shape[1], img.shape[0], br.DEFAULTS["levels"]))))
    print("intensity | bright pixels | bright share | increase of the mean luminance")
    for r in rows:
        print("%9.2f | %13d | %12.5f | %.5f" % (r["intensity"], r["bright_pixels"], r["bright_share"], r["increase"]))
    chosen = pick(rows)
    print("the largest intensity below %.0f %%: %s (the default is %s)" % (100 * LIMIT, chosen, br.DEFAULTS["intensity"]))
    if a.json:
        json.dump({"exposure": float(exposure), "rows": rows, "chosen": chosen}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
