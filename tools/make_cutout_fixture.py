#!/usr/bin/env python3
"""Writes the alpha-cutout fixtures of tests/golden/cutout/ (this repo's own files): three 8-bit opacity PNGs -- RGBA,
grey and grey + alpha -- a small sky, and a JSON scene in the reference's schema whose materials name them through the
"opacity" / "opacity-cutoff" keys.  tests/test_cutout.py recomputes the alpha bytes below and compares.

Usage: python tools/make_cutout_fixture.py [out_dir]"""
import json
import struct
import sys
import zlib
from pathlib import Path

import numpy as np


def write_png(path, a):
    """a: [h, w] or [h, w, c] uint8 with c in 1 (grey), 2 (grey + alpha), 3 (RGB), 4 (RGBA)"""
    a = np.asarray(a, np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b"")
    Path(path).write_bytes(png)


def leaf_alpha():
    """8 x 8: a disc of A = 255 on A = 0 with one soft ring"""
    yy, xx = np.mgrid[0:8, 0:8]
    r = np.hypot(xx - 3.5, yy - 3.5)
    return np.where(r < 2.6, 255, np.where(r < 3.6, 96, 0)).astype(np.uint8)


def fence_alpha():
    """5 x 3 grey: bars"""
    return np.array([[255, 0, 255, 0, 255], [255, 40, 255, 200, 255], [255, 0, 255, 0, 255]], np.uint8)


def decal_alpha():
    """4 x 4, stored as grey + alpha with a DIFFERENT grey: the loader must take the alpha byte"""
    return ((np.arange(16).reshape(4, 4) * 17) % 256).astype(np.uint8)


def scene():
    mat = lambda name, **kw: dict({"name": name, "diffuse": [0.7, 0.7, 0.7], "metallic": 0.0, "roughness": 0.8,
                                   "oren-nayar-dielectric": {"multiscatter-multiplier": 1.0}}, **kw)
    srt = lambda name, **kw: {"name": name, "srt": kw}
    return {
        "camera": {"focalLength": 24, "sensorSize": 36, "direction": [0, 1, -0.2], "max-depth": 6},
        "film": {"resolutionX": 32, "resolutionY": 32, "samples": 4},
        "textures": [{"name": "leaf", "type": "opacity", "path": "leaf_rgba_8x8.png"},
                     {"name": "fence", "type": "opacity", "path": "fence_grey_5x3.png"},
                     {"name": "decal", "type": "opacity", "path": "decal_ga_4x4.png"}],
        "materials": [mat("chalk"), mat("leafmat", opacity="leaf", **{"opacity-cutoff": 0.25}),
                      mat("fencemat", opacity="fence", **{"opacity-cutoff": 0.25}), mat("solid", diffuse=[0.8, 0.3, 0.2])],
        "objects": [{"name": "floor", "type": "primitive", "shape": "plane", "material": "chalk"},
                    {"name": "leafcard", "type": "primitive", "shape": "plane", "material": "leafmat"},
                    {"name": "fencecard", "type": "primitive", "shape": "plane", "material": "fencemat"},
                    {"name": "block", "type": "primitive", "shape": "cube", "material": "solid"}],
        "lights": [{"name": "bulb", "type": "point", "radiant-intensity": [9, 9, 8]}],
        "envlight": "sky_8x8.png",
        "transforms": [srt("room", **{"translation-vector": [0, 4, -1]}),
                       srt("ground", scale=[10, 10, 1], **{"translation-vector": [0, 0, -0.5]}),
                       srt("canopy", scale=[2, 2, 1], **{"translation-vector": [0, 0, 1.2]}),
                       srt("gate", scale=[2, 2, 1], **{"translation-vector": [-1, 0.5, 0.5], "rotate-axis": [1, 0, 0], "rotate-degrees": 80}),
                       srt("box", scale=0.6, **{"translation-vector": [0.9, 0.4, 0.0]}),
                       srt("lamp", **{"translation-vector": [0.2, 0.0, 3.0]})],
        "world": {"room": {"ground": {"instances": ["floor"]}, "canopy": {"instances": ["leafcard"]}, "gate": {"instances": ["fencecard"]},
                           "box": {"instances": ["block"]}, "lamp": {"lights": ["bulb"]}}},
    }


def main(out):
    out = Path(out)
    out.mkdir(parents=True, exist_ok=True)
    a = leaf_alpha()
    rgb = np.stack([np.full_like(a, 30), np.full_like(a, 160), np.full_like(a, 40)], -1)  # green: must NOT reach the texel store
    write_png(out / "leaf_rgba_8x8.png", np.concatenate([rgb, a[..., None]], -1))
    write_png(out / "fence_grey_5x3.png", fence_alpha())
    d = decal_alpha()
    write_png(out / "decal_ga_4x4.png", np.stack([255 - d, d], -1))
    yy, xx = np.mgrid[0:8, 0:8]
    write_png(out / "sky_8x8.png", np.stack([60 + 10 * yy, 80 + 12 * xx, np.full_like(xx, 150)], -1))
    (out / "cards.json").write_text(json.dumps(scene(), indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else Path(__file__).resolve().parent.parent / "tests" / "golden" / "cutout")
