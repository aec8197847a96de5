"""enerf_amd/render_path.py against the reference's scripts/render.py and utils/pose_utils.py (tests/golden/
ref_render_path.npz, minted by tests/refcheck/mint_view_golden.py from 12 seeded poses), and by its properties."""
import numpy as np
import pytest

from util import golden
from test_view_host import path_inputs


def _orthonormal(R, tol=1e-6):
    eye = np.einsum("nij,nkj->nik", R.astype(np.float64), R.astype(np.float64))
    assert np.abs(eye - np.eye(3)).max() < tol
    assert np.allclose(np.linalg.det(R.astype(np.float64)), 1.0, atol=tol)


def test_interpolate_poses_matches_the_reference():
    from enerf_amd.render_path import interpolate_poses
    g = golden("ref_render_path")
    poses, _ = path_inputs()
    i0, i1 = (int(v) for v in g["between_idx"])
    got = interpolate_poses(poses[i0], poses[i1], 7)
    assert got.shape == (8, 3, 4) and got.dtype == np.float32
    np.testing.assert_allclose(got, g["between"][:, :3, :4], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[0], poses[i0][:3], rtol=0, atol=1e-6)            # the end poses are reproduced
    np.testing.assert_allclose(got[-1], poses[i1][:3], rtol=0, atol=1e-6)
    _orthonormal(got[:, :, :3])
    # [3, 4] inputs too, and the ratio eases in and out: the first step is shorter than the middle one
    again = interpolate_poses(poses[i0][:3], poses[i1][:3], 7)
    assert np.array_equal(again, got)
    step = np.linalg.norm(np.diff(got[:, :, 3], axis=0), axis=1)
    assert step[0] < step[3] and abs(step[0] - step[-1]) < 1e-6
    with pytest.raises(ValueError):
        interpolate_poses(poses[0], poses[1], 0)


def test_spiral_poses_matches_the_reference():
    from enerf_amd.render_path import spiral_poses
    g = golden("ref_render_path")
    poses, _ = path_inputs()
    got = spiral_poses(poses)
    assert got.shape == (120, 3, 4) and got.dtype == np.float32
    np.testing.assert_allclose(got, g["spiral"][:, :3, :4], rtol=0, atol=1e-6)
    assert np.array_equal(spiral_poses(poses[:, :3, :4]), got)
    # the "hwf" column the reference carries along is pose 0's translation and is not part of the result
    np.testing.assert_allclose(g["spiral"][:, :, 4], np.tile(poses[0, :3, 3], (120, 1)), rtol=0, atol=1e-6)
    _orthonormal(got[:, :, :3], 1e-5)


def test_spiral_poses_properties():
    from enerf_amd.render_path import spiral_poses
    poses, _ = path_inputs()
    n, rots = 40, 2
    got = spiral_poses(poses, n_views=n, n_rots=rots).astype(np.float64)
    # closed after n_rots turns: at the same step, the pose at theta = 2 pi n_rots is the first one again
    more = spiral_poses(poses, n_views=2 * n, n_rots=2 * rots)
    np.testing.assert_allclose(more[:n], got, rtol=0, atol=1e-6)
    np.testing.assert_allclose(more[n], got[0], rtol=0, atol=1e-6)
    # positions: centre + x r0 cos(theta) - y r1 sin(theta) - z r2 sin(theta / 2) in the averaged frame
    p = poses[:, :3, :]
    center = p[:, :, 3].mean(0)
    rads = np.percentile(np.abs(p[:, :, 3]), 90, 0) * np.array([0.2, 0.2, 1.0])
    z = p[:, :, 2].sum(0)
    z /= np.linalg.norm(z)
    x = np.cross(p[:, :, 1].sum(0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    local = np.stack([(got[:, :, 3] - center) @ a for a in (x, y, z)], 1)
    theta = np.linspace(0, 2 * np.pi * rots, n + 1)[:-1]
    want = np.stack([np.cos(theta) * rads[0], -np.sin(theta) * rads[1], -np.sin(theta * 0.5) * rads[2]], 1)
    np.testing.assert_allclose(local, want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.abs(local).max(0)[:2], rads[:2], rtol=1e-2)
    with pytest.raises(ValueError):
        spiral_poses(np.zeros((3, 2, 4)))


def test_poses_from_quat_list_matches_the_reference():
    from enerf_amd.render_path import poses_from_quat_list
    g = golden("ref_render_path")
    _, quats = path_inputs()
    got = poses_from_quat_list(quats)
    assert got.shape == (5, 3, 4) and got.dtype == np.float32
    np.testing.assert_allclose(got, g["quat_poses"][:, :3, :4], rtol=0, atol=1e-6)
    assert np.array_equal(g["quat_poses"][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (5, 1)))
    np.testing.assert_allclose(got[:, :, 3], quats[:, 1:4], rtol=0, atol=1e-7)
    _orthonormal(got[:, :, :3])
    assert poses_from_quat_list(np.zeros((0, 8))).shape == (0, 3, 4)
    with pytest.raises(ValueError):
        poses_from_quat_list(np.zeros((2, 7)))
