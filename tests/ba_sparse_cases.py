"""Scenes for the sparse path of the bundle adjustment (tests/test_ba_sparse_host.py, tests/test_gpu_ba_sparse.py,
tools/ba_sparse_probe.py): the trajectory of conftest.make_ba_scene with a short sight, so that a keyframe shares points with a few
neighbours only, optionally with a loop; and a vectorised large map with tracks of four.  An ordinary module."""
import numpy as np

EDGE_DTYPE = np.dtype([("pose", np.int32), ("point", np.int32), ("stereo", np.int32), ("pad_", np.int32),
                       ("obs", np.float64, 3), ("inv_sigma2", np.float64)])
INTR = (718.856, 718.856, 498.692, 173.215, 386.1448)          # KITTI-00: fx fy cx cy bf


def windowed_scene(seed, n_kf, loop=0, stereo_frac=0.8):
    """Keyframes 1 m apart along z (yaw within 2 degrees), 12 points per metre of path in x [-6, 6], y [-2, 2], z [2, path + 9]; a point
    is seen when 2 < z_cam < 9 inside 1024 x 352.  loop = k: the last k keyframes stand at z = 0.5, 1.5, ... and see the start again.
    Returns poses (n_kf, 12), points, edges, intr as make_ba_scene does."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = INTR
    path = n_kf - loop
    poses = np.zeros((n_kf, 12))
    for k in range(n_kf):
        yaw = np.deg2rad(rng.uniform(-2, 2))
        Rwc = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        z = 1.0 * k if k < path else 0.5 + (k - path)
        twc = np.array([rng.normal(0, 0.05), rng.normal(0, 0.02), z])
        Rcw = Rwc.T
        poses[k, :9] = Rcw.ravel(); poses[k, 9:] = -Rcw @ twc
    n_pts = 12 * (path + 9)
    pts = np.stack([rng.uniform(-6, 6, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(2, path + 9, n_pts)], 1)
    edges = []
    for k in range(n_kf):
        R = poses[k, :9].reshape(3, 3); t = poses[k, 9:]
        pc = pts @ R.T + t
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * pc[:, 0] / z + cx; v = fy * pc[:, 1] / z + cy
        vis = (z > 2) & (z < 9) & (u >= 0) & (u < 1024) & (v >= 0) & (v < 352)
        for i in np.nonzero(vis)[0]:
            lvl = rng.integers(0, 8); sig = 1.2 ** lvl
            st = rng.random() < stereo_frac
            obs = [u[i] + rng.normal(0, sig), v[i] + rng.normal(0, sig), u[i] - bf / z[i] + rng.normal(0, sig)]
            if rng.random() < 0.02: obs[0] += 30          # outliers exercise the Huber branch
            edges.append((k, i, int(st), 0, obs, 1.0 / (sig * sig)))
    return poses, pts, np.array(edges, dtype=EDGE_DTYPE), INTR


def ring_scene(seed, n_kf, stereo_frac=0.8):
    """A loop that closes: keyframes 1 m apart on a circle (heading along the tangent, yaw within 2 degrees of it), 12 points per metre
    within 6 m of the path to either side, the sight and the observations of windowed_scene.  The keyframes of windowed_scene stand on a
    line, so the poses that share points form an interval graph, which a minimum-degree order factors without fill whatever `loop` is;
    on the circle the last keyframes see the first ones' points and the factor has blocks that S has not."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = INTR
    rad = n_kf / (2 * np.pi)
    poses = np.zeros((n_kf, 12))
    for k in range(n_kf):
        th = 2 * np.pi * k / n_kf
        yaw = th + np.deg2rad(rng.uniform(-2, 2))
        Rwc = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        twc = np.array([rad * (1 - np.cos(th)) + rng.normal(0, 0.05), rng.normal(0, 0.02), rad * np.sin(th)])
        Rcw = Rwc.T
        poses[k, :9] = Rcw.ravel(); poses[k, 9:] = -Rcw @ twc
    n_pts = 12 * n_kf
    phi = rng.uniform(0, 2 * np.pi, n_pts); rr = rad + rng.uniform(-min(6.0, 0.8 * rad), 6, n_pts)
    pts = np.stack([rad - rr * np.cos(phi), rng.uniform(-2, 2, n_pts), rr * np.sin(phi)], 1)
    edges = []
    for k in range(n_kf):
        R = poses[k, :9].reshape(3, 3); t = poses[k, 9:]
        pc = pts @ R.T + t
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * pc[:, 0] / z + cx; v = fy * pc[:, 1] / z + cy
        vis = (z > 2) & (z < 9) & (u >= 0) & (u < 1024) & (v >= 0) & (v < 352)
        for i in np.nonzero(vis)[0]:
            lvl = rng.integers(0, 8); sig = 1.2 ** lvl
            st = rng.random() < stereo_frac
            obs = [u[i] + rng.normal(0, sig), v[i] + rng.normal(0, sig), u[i] - bf / z[i] + rng.normal(0, sig)]
            if rng.random() < 0.02: obs[0] += 30
            edges.append((k, i, int(st), 0, obs, 1.0 / (sig * sig)))
    return poses, pts, np.array(edges, dtype=EDGE_DTYPE), INTR


def track_map(seed, n_kf, n_pts, track=4, noise=0.5):
    """A long straight map built without a Python loop over the edges: keyframe k at z = k (identity rotation), point q first seen by
    keyframe k0 = q * (n_kf - track + 1) // n_pts and by the `track` - 1 keyframes behind it, 3 to 6 m ahead of the last of them.
    Stereo observations with `noise` pixels of error.  Returns poses, points, edges, intr."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = INTR
    poses = np.zeros((n_kf, 12)); poses[:, [0, 4, 8]] = 1.0; poses[:, 11] = -np.arange(n_kf)
    k0 = (np.arange(n_pts, dtype=np.int64) * (n_kf - track + 1)) // n_pts
    depth = rng.uniform(3, 6, n_pts)                               # from the last keyframe of the track
    zc = depth + track - 1                                         # from the first
    pts = np.stack([rng.uniform(-0.4, 0.4, n_pts) * depth, rng.uniform(-0.15, 0.15, n_pts) * depth, k0 + zc], 1)
    kf = (k0[:, None] + np.arange(track)[None, :]).ravel()
    pt = np.repeat(np.arange(n_pts), track)
    z = pts[pt, 2] - kf
    u = fx * pts[pt, 0] / z + cx; v = fy * pts[pt, 1] / z + cy
    e = np.zeros(len(kf), EDGE_DTYPE)
    e["pose"] = kf; e["point"] = pt; e["stereo"] = 1; e["inv_sigma2"] = 1.0
    e["obs"] = np.stack([u, v, u - bf / z], 1) + rng.normal(0, noise, (len(kf), 3))
    return poses, pts, e, INTR


def start(poses, pts, n_fixed, seed, rot=0.002, trans=0.02, dx=0.05):
    """The perturbed start of tests/test_gpu_ba_solve.py: the first n_fixed keyframes fixed, the others moved, the points jittered."""
    from conftest import perturb_pose
    rng = np.random.default_rng(seed)
    fixed = np.zeros(len(poses), np.uint8); fixed[:n_fixed] = 1
    P0 = poses.copy()
    for i in range(n_fixed, len(poses)):
        P0[i] = perturb_pose(poses[i], rng, rot, trans)
    return P0, fixed, pts + rng.normal(0, dx, pts.shape)
