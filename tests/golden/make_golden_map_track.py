#!/usr/bin/env python3
"""Golden vectors for localization mode, produced by IMPORTING the reference.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_map_track.py

One track of 6 scans of 181 beams in `synth.Scene` at resolution 0.05, with an odometry that drifts a few centimetres and
about 0.02 rad per step, followed through the map by the loop of `ym_map_track`:

    prior_i = pose_{i-1} (+) ((-) odom_{i-1} (+) odom_i)                      graph_slam.py:320-324
    R       = the reference's own Scan2DMatcherPy.match_scan_sets_with_map(cgrid, ox, oy, [scan at prior_i], True, True)
    pose_i  = (R.x, R.y, prior_i.heading + R.heading)     the set's rigid correction; R = the corrected centre

`find_best_pose_non_symmetric` is bound into the wrapper's module as in make_golden_map.py (the import the reference forgot),
here through a recorder that keeps what each of its two calls per step returned; the function bodies that compute the fixture
are the reference's, unmodified.  The planar Transform stand-ins are make_golden_map.py's.

Checked here, so that the device test may compare poses: at no step does a hypothesis of the coarse pass reach the best integer
sum outside the best one's neighbourhood (3 lattice steps in x and y, 2 in heading) -- the tie mean then stays inside one basin.

Output: tests/golden/map_track.npz (inputs + the reference's outputs; data only).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_map as MM  # noqa: E402  (installs the stand-ins, imports the reference, binds the missing name)

MG, H, SM, synth = MM.MG, MM.H, MM.SM, MM.synth
T = MG.Transform

RES, SMEAR, N_BEAMS, MIN_RESPONSE = 0.05, 0.05, 181, 0.0
TRUTH = [(3.00, 3.00, 0.00), (3.12, 3.02, 0.03), (3.25, 3.05, 0.07), (3.37, 3.10, 0.12), (3.48, 3.16, 0.16), (3.58, 3.24, 0.21)]
DRIFT = (0.03, -0.02, 0.02)  # per step, added to the true increment in the previous scan's frame

_calls = []


def _recorder(*a, **k):
    out = H.find_best_pose_non_symmetric(*a, **k)
    _calls.append(np.array(out, dtype=np.float64))
    return out


SM.find_best_pose_non_symmetric = _recorder


def _coarse_ties_stay_in_one_basin(cgrid, scan, ox, oy):
    p = scan.corrected_pose
    xl, yl = H._transform_points(*scan.points(), -p.x, -p.y, 0)
    xv, yv, tv = (np.arange(-0.25 + p.x, 0.25 + p.x, 0.01), np.arange(-0.25 + p.y, 0.25 + p.y, 0.01), np.arange(-0.1, 0.1, 0.01))
    vol = np.zeros((len(tv), len(yv), len(xv)), dtype=np.int64)
    for k, t in enumerate(tv):
        xx, yy = H._rotate_points(xl, yl, t)
        gx = np.round(((xv[:, None] + xx[None, :]) - ox) / 0.05).astype(np.int64)  # helpers.py:149-153, per (hypothesis, point) pair
        gy = np.round(((yv[:, None] + yy[None, :]) - oy) / 0.05).astype(np.int64)
        okx, oky = (gx >= 0) & (gx < cgrid.shape[1]), (gy >= 0) & (gy < cgrid.shape[0])
        g100 = (100 * cgrid).astype(np.int64)
        for j in range(len(yv)):
            ok = okx & oky[j][None, :]
            vol[k, j] = np.where(ok, g100[np.clip(gy[j], 0, cgrid.shape[0] - 1)[None, :], np.clip(gx, 0, cgrid.shape[1] - 1)], 0).sum(axis=1)
    best = np.argwhere(vol == vol.max())
    span = best.max(axis=0) - best.min(axis=0)
    assert span[0] <= 2 and span[1] <= 3 and span[2] <= 3, "the best coarse sum is reached in more than one basin: %s" % best


def main():
    scene = synth.Scene()
    ox, oy = -0.6, -0.45
    w, h = int((scene.width + 1.2) / RES) + 3, int((scene.height + 0.9) / RES) + 2
    im = MM.occupancy_image(scene, RES, ox, oy, w, h)
    cgrid = H.occupancy_grid_map_to_correlation_grid(im, RES, SMEAR, 0)
    sensor = dict(min_angle=synth.MIN_ANGLE, angle_increment=synth.ANGLE_INCREMENT * (1081 - 1) / (N_BEAMS - 1),
                  min_range=synth.MIN_RANGE, range_threshold=12.0)
    ranges = [scene.scan_ranges(t, index=700 + i, n_beams=N_BEAMS, min_angle=sensor["min_angle"], inc=sensor["angle_increment"])
              for i, t in enumerate(TRUTH)]
    # odometry: the true increments, each with the drift added in the previous scan's frame
    odom = [T(*TRUTH[0])]
    for a, b in zip(TRUTH, TRUTH[1:]):
        inc = T(*b) - T(*a)
        odom.append(odom[-1] + T(inc.x + DRIFT[0], inc.y + DRIFT[1], inc.euler[-1] + DRIFT[2]))
    m = SM.Scan2DMatcherPy(dict(resolution=RES, smear_deviation=SMEAR, range_threshold=12.0))
    poses = [T(*TRUTH[0])]
    priors, coarse, fine, responses, covs, accepted = [], [], [], [], [], []
    for i in range(1, len(TRUTH)):
        prior = poses[-1] + (odom[i] - odom[i - 1])
        scan = MG.RefScan(ranges[i], sensor, (prior.x, prior.y, prior.euler[-1]))
        _coarse_ties_stay_in_one_basin(cgrid, scan, ox, oy)
        del _calls[:]
        r = m.match_scan_sets_with_map(cgrid, ox, oy, [scan], True, True)
        assert len(_calls) == 2 and float(r.response) == float(_calls[1][0])
        R = _calls[1]
        ok = float(r.response) >= MIN_RESPONSE
        pose = T(R[1], R[2], prior.euler[-1] + R[3]) if ok else prior
        priors.append([prior.x, prior.y, prior.euler[-1]])
        coarse.append(_calls[0]); fine.append(_calls[1])
        responses.append(float(r.response)); covs.append(np.array(r.covariance, dtype=np.float64)); accepted.append(int(ok))
        poses.append(pose)
        print("step %d prior (%.5f, %.5f, %.5f) response %.9f -> pose (%.5f, %.5f, %.5f)  truth (%.2f, %.2f, %.2f)" % (
            (i, prior.x, prior.y, prior.euler[-1], r.response, pose.x, pose.y, pose.euler[-1]) + TRUTH[i]))
    np.savez_compressed(
        os.path.join(HERE, "map_track.npz"),
        image=im, res=RES, smear=SMEAR, ox=ox, oy=oy, min_response=MIN_RESPONSE,
        sensor_min_angle=sensor["min_angle"], sensor_angle_increment=sensor["angle_increment"],
        sensor_min_range=sensor["min_range"], sensor_range_threshold=sensor["range_threshold"],
        ranges=np.array(ranges), odom=np.array([[o.x, o.y, o.euler[-1]] for o in odom]), start_pose=np.array(TRUTH[0]),
        priors=np.array(priors), coarse=np.array(coarse), fine=np.array(fine), responses=np.array(responses),
        covariances=np.array(covs), accepted=np.array(accepted, dtype=np.int32),
        poses=np.array([[p.x, p.y, p.euler[-1]] for p in poses]))


if __name__ == "__main__":
    main()
