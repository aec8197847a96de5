"""The event side of collate with `accumulate_evs = 0` on the host (enerf_amd/event_sampler.py):
the statements -- sample_event_pairs(accumulate=False) + PoseTrack.poses_at + get_event_rays -- against the reference's
own collate of that branch (tests/golden/ref_collate.npz `single_*`), and EventSampler.batch on CPU tables, which runs
them.  The device kernels are held to the same statements in test_gpu_event_sampler_direct.py."""
import numpy as np
import pytest
import torch

from util import golden

INTR = (14.0, 13.0, 8.0, 6.0)
RAYS = ("rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2")


@pytest.fixture(scope="module")
def z():
    return golden("ref_collate")


def _tables_and_track(z, dev="cpu"):
    from enerf_amd.event_sampler import build_event_tables
    from enerf_amd.pose_interp import PoseTrack
    t = build_event_tables(torch.from_numpy(z["events"]).to(dev))
    return t, PoseTrack(z["pose_ts"], z["pose_R"], z["pose_t"], device=dev)


def single_draws(z, tables):
    """The fixture's draws of the accumulate_evs = 0 branch as the restatement takes them: np.random.rand(P), and the
    positions of np.random.choice's chosen event ids among the per-pixel events."""
    u_xy = z["single_draw_rand_first"]
    chosen = z["single_draw_choice_first"].astype(np.int64)
    per_pixel = (u_xy * tables["num_at_xy"].cpu().numpy() - 1).astype(int) + tables["first_at_xy"].cpu().numpy()
    pos = np.array([int(np.nonzero(per_pixel == c)[0][0]) for c in chosen])
    return {"u_xy": torch.from_numpy(u_xy), "choice": torch.from_numpy(pos)}, chosen


def no_event_case(z, dev="cpu"):
    """The `acc_noev` collate's no-event draws and tables, as test_collate_vs_reference takes them (n = 32)."""
    rest = z["acc_noev_draw_randint_rest"]
    chunk, idx = int(rest[64]), rest[65:65 + 32].astype(np.int64)
    u = z["acc_noev_draw_random_first"]
    n = int(z["noev_n_chunks"])
    no_evs = {"coords": [torch.from_numpy(z[f"noev_coords{j}"]).to(dev) for j in range(n)], "N_ev_chunks": n,
              "start_time_us": z["noev_start_us"].tolist(), "end_time_us": z["noev_end_us"].tolist()}
    return no_evs, {"chunk": chunk, "idx": torch.from_numpy(idx), "u": torch.from_numpy(u)}


def test_statements_equal_the_reference_collate_of_the_direct_successor_branch(z):
    from enerf_amd.event_sampler import sample_event_pairs
    from enerf_amd.events import get_event_rays
    t, track = _tables_and_track(z)
    draws, chosen = single_draws(z, t)
    s, e, p, xs, ys = sample_event_pairs(t, 64, False, draws=draws)
    assert np.array_equal(s.numpy(), chosen) and np.array_equal(e.numpy(), chosen + 1)
    assert np.array_equal(p.numpy(), z["single_pols"])
    ev = t["events"]
    rays = get_event_rays(xs, ys, track.poses_at(ev[s, 2]).unsqueeze(0), track.poses_at(ev[e, 2]).unsqueeze(0), INTR)
    for k in RAYS:
        print(f"{k}: max |statement - reference| = {np.abs(rays[k].numpy() - z['single_' + k]).max():.3e}")
        np.testing.assert_allclose(rays[k].numpy(), z[f"single_{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


def test_cpu_sampler_with_the_fixture_draws_is_the_statement(z):
    from enerf_amd.event_sampler import EventSampler
    t, track = _tables_and_track(z)
    draws, chosen = single_draws(z, t)
    b = EventSampler([t], track, INTR, 64, seed=0).batch([0], draws=draws)
    assert np.array_equal(b["start"].numpy(), chosen) and np.array_equal(b["pols"].numpy(), z["single_pols"])
    for k in RAYS:
        np.testing.assert_allclose(b[k].numpy(), z[f"single_{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


def _events(n, w, h, seed):
    rng = np.random.default_rng(seed)
    ts = rng.permutation(n * 3)[:n].astype(np.float64) * 1000.0
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n), ts, rng.choice([-1.0, 1.0], n)], 1).astype(np.float32)


def _track(K, t_lo, t_hi, seed):
    from scipy.spatial.transform import Rotation
    from enerf_amd.pose_interp import PoseTrack
    rng = np.random.default_rng(seed)
    t = np.linspace(t_lo - 1.0, t_hi + 1.0, K)
    R = Rotation.from_rotvec(np.cumsum(rng.normal(size=(K, 3)) * 0.04, 0))
    p = np.cumsum(rng.normal(size=(K, 3)) * 0.02, 0) + np.array([1.5, 0.3, 0.0])
    return PoseTrack(t, R.as_matrix(), p)


def _frames(H, W, n, V=2):
    from enerf_amd.frame_sampler import FrameSampler
    poses = torch.eye(4).repeat(V, 1, 1)
    poses[:, :3, 3] = torch.arange(V * 3, dtype=torch.float32).view(V, 3) * 0.1
    g = torch.Generator().manual_seed(1)
    return FrameSampler(poses, (30.0, 30.0, W / 2, H / 2), H, W, images=torch.rand(V, H, W, 3, generator=g), num_rays=n)


def test_cpu_sampler_batch_is_the_data_dict_of_the_event_step():
    from enerf_amd.event_sampler import EventSampler, build_no_event_tables
    W, H, M = 20, 15, 128
    evs = [torch.from_numpy(_events(2500, W, H, 3 + v)) for v in range(2)]
    track = _track(12, 0.0, 7.5e6, 5)
    span = (float(evs[0][:, 2].min()) * 1e-3, float(evs[0][:, 2].max()) * 1e-3)
    no_evs = [build_no_event_tables(e, H, W, *span) for e in evs]
    s = EventSampler(evs, track, (30.0, 30.0, 10.0, 7.5), M, no_events=no_evs, frames=_frames(H, W, 16), seed=4)
    b = s.batch([1])
    for k in RAYS:
        assert b[k].shape == (1, M, 3) and b[k].dtype == torch.float32, k
        assert b[k.replace("evs", "no_evs")].shape == (1, M // 2, 3) and b[k.replace("evs", "no_evs")].dtype == torch.float32
    assert b["pols"].shape == (1, M) and b["pols"].dtype == torch.float32
    assert b["rays_o"].shape == b["rays_d"].shape == (1, 16, 3) and b["images"].shape == (1, 16, 3)
    assert b["index"] == [1] and (b["H"], b["W"]) == (H, W)
    assert b["start"].dtype == b["end"].dtype == torch.int64 and b["tss_us"].shape == (M // 2, 2)
    # the reference's data dict of this branch (provider.py:1412-1500), all present
    assert {"rays_evs_o1", "rays_evs_d1", "rays_evs_o2", "rays_evs_d2", "pols", "rays_no_evs_o1", "rays_no_evs_d1",
            "rays_no_evs_o2", "rays_no_evs_d2", "rays_o", "rays_d", "images", "index", "H", "W"} <= set(b)
    # direct successors at one pixel, M <= P distinct pixels
    ev = s.tables[1]["events"]
    st, en = b["start"], b["end"]
    assert torch.equal(en, st + 1) and torch.equal(ev[st, :2], ev[en, :2]) and bool((ev[st, 2] < ev[en, 2]).all())
    assert torch.equal(b["pols"][0], ev[en, 3])
    P = s.tables[1]["num_at_xy"].shape[0]
    assert M <= P and len({(float(x), float(y)) for x, y in ev[st, :2]}) == M
    # seeded: the same sampler state gives the same batch, the next draw another
    again = EventSampler(evs, track, (30.0, 30.0, 10.0, 7.5), M, no_events=no_evs, frames=_frames(H, W, 16), seed=4)
    b2 = again.batch([1])
    assert torch.equal(b2["start"], st) and torch.equal(b2["rays_no_evs_d2"], b["rays_no_evs_d2"]) and b2["chunk"] == b["chunk"]
    assert not torch.equal(again.batch([1])["start"], st)
    # more pairs than pixels: drawn with replacement
    many = EventSampler(evs, track, (30.0, 30.0, 10.0, 7.5), P + 7, seed=1).batch([1])
    assert many["rays_evs_o1"].shape == (1, P + 7, 3) and len(set(many["start"].tolist())) < P + 7
    # without a frame sampler: the empty images the event-only step reads the batch size from
    assert many["images"].shape == (1, 0, 3) and "rays_o" not in many and "H" not in many
    with pytest.raises(ValueError):
        s.batch([2])


def test_cpu_sampler_forwards_accumulate_evs_to_the_accumulate_statement():
    from enerf_amd.event_sampler import EventSampler, build_event_tables, sample_event_pairs
    from enerf_amd.events import get_event_rays
    ev = torch.from_numpy(_events(2500, 20, 15, 8))
    t = build_event_tables(ev)
    track = _track(12, 0.0, 7.5e6, 5)
    N, M = t["events"].shape[0], 96
    g = torch.Generator().manual_seed(2)
    draws = {"start": torch.randint(0, N, (M,), generator=g), "u_end": torch.rand(M, generator=g, dtype=torch.float64)}
    b = EventSampler(t, track, INTR, M, accumulate_evs=1, acc_max_num_evs=3, seed=0).batch(0, draws=draws)
    s, e, p, xs, ys = sample_event_pairs(t, M, True, 3, draws=draws)
    assert torch.equal(b["start"], s) and torch.equal(b["end"], e) and torch.equal(b["pols"], p)
    assert int((e - s).max()) > 1 and int((e - s).max()) <= 4
    ts = t["events"][:, 2]
    ref = get_event_rays(xs, ys, track.poses_at(ts[s]).unsqueeze(0), track.poses_at(ts[e]).unsqueeze(0), INTR)
    for k in RAYS:
        assert torch.equal(b[k], ref[k]), k


def test_the_one_launch_wrappers_raise_on_cpu_tables(z):
    from enerf_amd.event_sampler import event_single_pair_rays, no_event_pair_rays
    t, track = _tables_and_track(z)
    with pytest.raises(RuntimeError, match="runs on the device"):
        event_single_pair_rays(t, track, INTR, 64)
    no_evs, draws = no_event_case(z)
    with pytest.raises(RuntimeError, match="runs on the device"):
        no_event_pair_rays(no_evs, track, INTR, 64, draws=draws)


def test_sampler_is_exported_from_the_package():
    import enerf_amd
    from enerf_amd.event_sampler import EventSampler
    from enerf_amd.frame_sampler import FrameSampler
    assert enerf_amd.EventSampler is EventSampler and enerf_amd.FrameSampler is FrameSampler
