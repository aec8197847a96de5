"""Camera paths for `TrainHarness.render_path`: the ones the reference's scripts/render.py renders along, on the host in
numpy fp64 like there.  Every function returns cam2world poses [n, 3, 4] float32.

    interpolate_poses(pose0, pose1, n)      interpol_traj_between_rand_poses (:219-239) between two GIVEN poses: n + 1 poses,
                                            ratio_i = sin((i / n - 0.5) pi) 0.5 + 0.5 (ease in and out), rotation by scipy's
                                            Slerp at that ratio, translation linear in it
    spiral_poses(poses, ...)                compute_render_poses (:280-317) with utils/pose_utils.py:372-422 normalize /
                                            viewmatrix / poses_avg and render_path_spiral (:267-278)
    poses_from_quat_list(rows)              utils/pose_utils.py:43-53, rows [t, px, py, pz, qx, qy, qz, qw]

spiral_poses, as the reference computes it: centre = the mean translation; z = the normalised sum of the poses' third
columns, up = the sum of their second columns, the averaged frame = viewmatrix(z, up, centre) = [x | y | z | centre] with
x = normalize(up x z), y = normalize(z x x); close = 0.9 mind, inf = 5 maxd, focal = 1 / (0.25 / close + 0.75 / inf); radii
= the 90th percentile of |translation| per axis, the first two scaled by rad_scale; for theta in n_views steps of
[0, 2 pi n_rots): c = frame . ((cos theta, -sin theta, -sin(theta / 2), 1) * (radii, 1)), looking direction
normalize(c - frame . (0, 0, -focal, 1)), pose = viewmatrix(that, normalize(up), c).  Its quirks are kept: the radii are
percentiles of the WORLD translations, not of translations relative to the centre; and the fifth ("hwf") column poses_avg
takes from a [N, 3, 4] input is pose 0's translation, which rides along and is cut off again by the result's [:, :3, :4].
"""
import numpy as np


def _unit(v):
    """Rows of v [..., 3] scaled to length 1."""
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _look_frames(forward, up, origin):
    """Camera frames [n, 3, 4] = [right | true up | forward | origin]: forward [n, 3] is where each camera looks, right is
    perpendicular to `up` [3] and forward, true up completes the right-handed triad."""
    fwd = _unit(forward)
    right = _unit(np.cross(np.broadcast_to(up, fwd.shape), fwd))
    true_up = _unit(np.cross(fwd, right))
    return np.stack([right, true_up, fwd, np.asarray(origin, np.float64)], axis=-1)


def _poses(poses, least):
    p = np.asarray(poses, np.float64)
    if p.ndim != 3 or p.shape[0] < least or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"poses {p.shape}: [n >= {least}, 3 or 4, 4] expected")
    return p[:, :3, :]


def interpolate_poses(pose0, pose1, n):
    from scipy.spatial.transform import Rotation, Slerp
    ends = _poses(np.stack([np.asarray(pose0, np.float64)[:3], np.asarray(pose1, np.float64)[:3]]), 2)
    n = int(n)
    if n < 1:
        raise ValueError(f"interpolate_poses: n = {n}")
    ratio = np.sin((np.arange(n + 1) / n - 0.5) * np.pi) * 0.5 + 0.5          # eases in and out of the two ends
    out = np.empty((n + 1, 3, 4))
    out[:, :, :3] = Slerp([0.0, 1.0], Rotation.from_matrix(ends[:, :, :3]))(ratio).as_matrix()
    out[:, :, 3] = ends[0, :, 3] + ratio[:, None] * (ends[1, :, 3] - ends[0, :, 3])
    return out.astype(np.float32)


def spiral_poses(poses, mind=0.9, maxd=1.2, rad_scale=0.2, n_views=120, n_rots=2):
    p = _poses(poses, 1)
    where = p[:, :, 3]
    up_sum = p[:, :, 1].sum(0)
    # the averaged camera: at the mean position, looking along the summed viewing directions
    right, true_up, ahead, centre = np.moveaxis(_look_frames(p[:, :, 2].sum(0)[None], up_sum, where.mean(0)[None])[0], 1, 0)
    # the point every pose of the spiral looks at: `focus` in front of the averaged camera, between the near and far depths
    near, far = 0.9 * mind, 5.0 * maxd
    focus = 1.0 / (0.25 / near + 0.75 / far)
    target = centre - focus * ahead
    radii = np.percentile(np.abs(where), 90, axis=0) * np.array([rad_scale, rad_scale, 1.0])
    theta = 2.0 * np.pi * n_rots * np.arange(int(n_views)) / int(n_views)
    offsets = np.stack([radii[0] * np.cos(theta), -radii[1] * np.sin(theta), -radii[2] * np.sin(0.5 * theta)], axis=1)
    origin = centre + offsets @ np.stack([right, true_up, ahead])
    return _look_frames(origin - target, _unit(up_sum), origin).astype(np.float32)


def poses_from_quat_list(rows):
    from scipy.spatial.transform import Rotation
    r = np.asarray(rows, np.float64)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"rows {r.shape}: [n, 8] = t, px, py, pz, qx, qy, qz, qw expected")
    out = np.zeros((r.shape[0], 3, 4))
    if r.shape[0]:
        out[:, :, :3] = Rotation.from_quat(r[:, 4:]).as_matrix()
        out[:, :, 3] = r[:, 1:4]
    return out.astype(np.float32)
