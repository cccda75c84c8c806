#!/usr/bin/env python3
"""Writes tests/golden/medium_grid_plume_8.npy: an 8 x 8 x 8 density grid (shape (nz, ny, nx), float32) for the
heterogeneous medium (dmt_set_medium_grid) -- a plume that widens and thins with height, inside a border
of empty voxels, so that the support box is smaller than the grid: x and y in 1 .. 6, z in 1 .. 7.

Usage: python tools/make_medium_grid_fixture.py"""
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "medium_grid_plume_8.npy"


def plume(n=8):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    cx = cy = (n - 1) / 2
    h = (z - 1) / (n - 2)                                 # 0 at the plume's foot (z = 1), 1 at the top voxel layer
    radius = 0.9 + 2.0 * h                                # it widens with height
    r2 = (x - cx) ** 2 + (y - cy) ** 2
    d = 2.0 * (1.0 - 0.6 * h) * np.exp(-r2 / (2 * radius ** 2))  # and thins
    d[r2 > 2.6 ** 2] = 0                                  # nothing outside x, y in 1 .. 6
    d[z < 1] = 0                                          # an empty layer under the foot
    return np.round(d, 3).astype("<f4")


if __name__ == "__main__":
    g = plume()
    np.save(OUT, g)
    pos = np.argwhere(g > 0)
    print(f"{OUT}: shape {g.shape}, {OUT.stat().st_size} bytes, {pos.shape[0]} voxels > 0, max {g.max()}, "
          f"support z {pos[:, 0].min()}..{pos[:, 0].max()} y {pos[:, 1].min()}..{pos[:, 1].max()} x {pos[:, 2].min()}..{pos[:, 2].max()}")
