#!/usr/bin/env python3
"""Golden vector for maps that take scans, produced by IMPORTING the reference.

Run in the build container only (needs the reference tree):

    python tests/golden/make_golden_map_grow.py

Two scans of 91 beams in `synth.Scene` (the second with NaN and over-range readings) at resolution 0.05 / smear 0.05 go into a
130 x 67 grid that covers the room's upper left part only, so that most readings fall outside, beyond its right side and below
it (negative rows): the reference's own scan model gives the world points (`points()`), the
reference's `world_to_grid` the cells (cast to int32 as scan_matching.py:82-84 does), its `calculate_kernel` the taps and its
`add_scan_to_grid` the grid.  Same throw-away stand-ins for numba / karto_scanmatcher / tiny_tf / cv2 as make_golden.py; the
function bodies that compute the fixture are the reference's, unmodified.

Output: tests/golden/map_grow.npz (inputs + the reference's outputs; data only; nonzero cells stored sparsely).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_map as MM  # noqa: E402  (installs the stand-ins, imports the reference)

MG, H, synth = MM.MG, MM.H, MM.synth

RES, SMEAR, N_BEAMS, W, HGT = 0.05, 0.05, 91, 130, 67
OX, OY = -0.213, 2.871
POSES = [(3.0, 3.0, 0.0), (4.6, 2.4, 1.9)]


def main():
    scene = synth.Scene()
    sensor = dict(min_angle=synth.MIN_ANGLE, angle_increment=synth.ANGLE_INCREMENT * (1081 - 1) / (N_BEAMS - 1),
                  min_range=synth.MIN_RANGE, range_threshold=12.0)
    ranges = [scene.scan_ranges(p, index=900 + i, n_beams=N_BEAMS, min_angle=sensor["min_angle"], inc=sensor["angle_increment"],
                                dirty=(i == 1)) for i, p in enumerate(POSES)]
    kernel = H.calculate_kernel(RES, SMEAR)
    cgrid = np.zeros((HGT, W))
    px, py, gxs, gys = [], [], [], []
    for r, p in zip(ranges, POSES):
        x, y = MG.RefScan(r, sensor, p).points()
        gx, gy = H.world_to_grid((np.array(x), np.array(y)), OX, OY, RES)
        gx, gy = gx.astype("int32"), gy.astype("int32")
        H.add_scan_to_grid(gx, gy, cgrid, kernel)
        px.append(x); py.append(y); gxs.append(gx); gys.append(gy)
    px, py, gxs, gys = (np.concatenate(v) for v in (px, py, gxs, gys))
    inside = (gxs >= 0) & (gxs < W) & (gys >= 0) & (gys < HGT)
    nzy, nzx = np.nonzero(cgrid)
    np.savez_compressed(
        os.path.join(HERE, "map_grow.npz"),
        res=RES, smear=SMEAR, ox=OX, oy=OY, width=W, height=HGT,
        sensor_min_angle=sensor["min_angle"], sensor_angle_increment=sensor["angle_increment"],
        sensor_min_range=sensor["min_range"], sensor_range_threshold=sensor["range_threshold"],
        ranges=np.array(ranges), poses=np.array(POSES, dtype=np.float64), kernel=kernel,
        points_x=px, points_y=py, gx=gxs, gy=gys, stamped=int(inside.sum()), dropped=int((~inside).sum()),
        cgrid_nz_y=nzy.astype(np.int32), cgrid_nz_x=nzx.astype(np.int32), cgrid_nz_val=cgrid[nzy, nzx])
    print("map_grow: %d points, %d stamped, %d dropped, %d nonzero cells" % (len(px), inside.sum(), (~inside).sum(), len(nzy)))


if __name__ == "__main__":
    main()
