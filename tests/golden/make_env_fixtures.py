#!/usr/bin/env python3
"""Generate the environment-map reader fixtures under tests/golden/env/ (tests/test_environment_host.py):

    flat.hdr   Radiance RGBE, 7 x 5, flat scanlines (width < 8 cannot be run-length encoded)
    rle.hdr    Radiance RGBE, 40 x 6, run-length encoded scanlines with both runs and literals
    grey.pfm   Pf, 9 x 4, little-endian
    colour.pfm PF, 6 x 3, big-endian
    expected.npz  the float32 [H, W, 3] each file decodes to (row 0 = the top row)

Written from fixed RGBE bytes and floats (no randomness beyond a fixed seed), so that the expected values are exact.

    python tests/golden/make_env_fixtures.py
"""
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "env")


def rgbe_to_float(px):
    e = px[..., 3:4].astype(np.int32)
    return np.where(e > 0, np.ldexp(px[..., :3].astype(np.float32), e - 136), 0).astype(np.float32)


def rle_plane(vals):
    """Radiance's scanline encoding of one component: runs of >= 4 equal bytes as (128 + n, v), the rest as literals (n, bytes)"""
    out, i, n = bytearray(), 0, len(vals)
    while i < n:
        j = i
        while j < n and vals[j] == vals[i] and j - i < 127:
            j += 1
        if j - i >= 4:
            out += bytes([128 + j - i, vals[i]])
            i = j
            continue
        k = i
        while k < n and k - i < 128:
            if k + 3 < n and vals[k] == vals[k + 1] == vals[k + 2] == vals[k + 3]:
                break
            k += 1
        out += bytes([k - i]) + bytes(vals[i:k])
        i = k
    return bytes(out)


def main():
    os.makedirs(HERE, exist_ok=True)
    rng = np.random.default_rng(16)
    exp = {}
    # flat .hdr
    px = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    px[..., 3] = rng.integers(120, 140, size=(5, 7))
    px[0, 0, 3] = 0                                           # a black texel
    with open(os.path.join(HERE, "flat.hdr"), "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 5 +X 7\n" + px.tobytes())
    exp["flat.hdr"] = rgbe_to_float(px)
    # run-length encoded .hdr
    px = rng.integers(0, 256, size=(6, 40, 4), dtype=np.uint8)
    px[:, 10:25] = px[:, 10:11]                               # runs
    px[..., 3] = np.clip(px[..., 3] % 16 + 125, 0, 255)
    body = bytearray()
    for y in range(6):
        body += bytes([2, 2, 0, 40])
        for c in range(4):
            body += rle_plane(list(px[y, :, c]))
    with open(os.path.join(HERE, "rle.hdr"), "wb") as f:
        f.write(b"#?RGBE\nFORMAT=32-bit_rle_rgbe\n\n-Y 6 +X 40\n" + bytes(body))
    exp["rle.hdr"] = rgbe_to_float(px)
    # grey .pfm, little-endian (negative scale); rows stored bottom first
    g = rng.uniform(0, 4, size=(4, 9)).astype(np.float32)
    with open(os.path.join(HERE, "grey.pfm"), "wb") as f:
        f.write(b"Pf\n9 4\n-1.0\n" + g[::-1].astype("<f4").tobytes())
    exp["grey.pfm"] = np.repeat(g[..., None], 3, axis=2)
    # colour .pfm, big-endian
    c = rng.uniform(0, 100, size=(3, 6, 3)).astype(np.float32)
    with open(os.path.join(HERE, "colour.pfm"), "wb") as f:
        f.write(b"PF\n6 3\n1.0\n" + c[::-1].astype(">f4").tobytes())
    exp["colour.pfm"] = c
    np.savez(os.path.join(HERE, "expected.npz"), **{k.replace(".", "_"): v for k, v in exp.items()})


if __name__ == "__main__":
    main()
