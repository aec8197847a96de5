"""The event side of collate with `accumulate_evs = 0` on the device (enerf_amd/event_sampler.py, csrc/event_pairs.hip,
DESIGN.md section 4.13): k_event_single_pair_rays and k_no_event_rays against the reference's own collate (the
`single_*` / `acc_noev_rays_no_evs_*` fixtures of tests/golden/ref_collate.npz), against the loop restatement with
scipy's interpolators at the smallest shapes where they can go wrong, their counters, EventSampler.batch against the CPU
sampler, and three event steps of TrainHarness fed by the sampler."""
import copy

import numpy as np
import pytest
import torch

from oracle import event_collate as EC
from test_event_sampler import _events, _track
from test_event_sampler_direct import INTR, RAYS, _tables_and_track, no_event_case, single_draws
from util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_RAYS = tuple(k.replace("evs", "no_evs") for k in RAYS)
ATOL = 2e-6            # the bound of the accumulate kernel in test_event_sampler.py: fp32 roundings of a unit vector's rotation


@pytest.fixture(scope="module")
def z():
    return golden("ref_collate")


# ------------------------------------------------------------------------------------------------ 1. the fixtures
def test_direct_pairs_equal_the_reference_collate(z):
    from enerf_amd.event_sampler import event_single_pair_rays
    t, track = _tables_and_track(z, DEV)
    draws, chosen = single_draws(z, t)
    assert t["num_at_xy"].shape[0] == 183 and track.K == 24
    r = event_single_pair_rays(t, track, INTR, 64, draws=draws)
    assert np.array_equal(r["start"].cpu().numpy(), chosen) and np.array_equal(r["end"].cpu().numpy(), chosen + 1)
    assert np.array_equal(r["pols"].cpu().numpy(), z["single_pols"])
    assert int(r["outside_track"]) == 0 and int(r["bad_choice"]) == 0
    for k in RAYS:
        print(f"{k}: max |kernel - reference| = {np.abs(r[k].cpu().numpy() - z['single_' + k]).max():.3e}")
        np.testing.assert_allclose(r[k].cpu().numpy(), z[f"single_{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


def test_no_event_rays_equal_the_reference_collate(z):
    from enerf_amd.event_sampler import no_event_pair_rays
    _, track = _tables_and_track(z, DEV)
    no_evs, draws = no_event_case(z, DEV)
    r = no_event_pair_rays(no_evs, track, INTR, 64, draws=draws)
    assert r["chunk"] == draws["chunk"] and int(r["outside_track"]) == 0 and int(r["bad_index"]) == 0
    for k in NO_RAYS:
        assert r[k].shape == (1, 32, 3)
        print(f"{k}: max |kernel - reference| = {np.abs(r[k].cpu().numpy() - z['acc_noev_' + k]).max():.3e}")
        np.testing.assert_allclose(r[k].cpu().numpy(), z[f"acc_noev_{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ 2. synthetic, pairs
SENSOR = (40, 30)
INTR_S = (35.0, 34.0, 19.5, 14.5)


@pytest.fixture(scope="module")
def synth():
    """5000 events on 40 x 30: the loop restatement's grouping and the device tables (equal, entry for entry)."""
    from enerf_amd.event_sampler import build_event_tables
    ev = _events(5000, *SENSOR, 12)
    g = EC.group_events(ev)
    tables = build_event_tables(torch.from_numpy(ev).to(DEV))
    assert np.array_equal(tables["events"].cpu().numpy(), g["events"])
    assert np.array_equal(tables["num_at_xy"].cpu().numpy(), g["xy_numEvs_Idx"][:, 0])
    return ev, g, tables


def _scipy_track(K, lo, hi, seed):
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Slerp
    from enerf_amd.pose_interp import PoseTrack
    t, R, p = _track(K, lo, hi, seed)
    track = PoseTrack(t, R.as_matrix(), p, device=DEV)
    return track, Slerp(t, R), interp1d(x=t, y=p, axis=0, kind="cubic", bounds_error=True), t


def _host_pose(slerp, cubic, ts):
    """provider.py:1411-1415: scipy at the event times, fp32 as torch.Tensor(get_hom_trafos(...)) rounds it."""
    ts = np.asarray(ts, np.float64)
    return torch.Tensor(np.concatenate([slerp(ts).as_matrix(), cubic(ts)[:, :, None]], -1)).unsqueeze(0)


def _cut(track, K2):
    """The first K2 knots of a track with the SAME per-segment tables (a PoseTrack built from fewer knots would fit another
    spline): what lies inside is evaluated exactly as before."""
    short = copy.copy(track)
    short.knots, short.rot = track.knots[:K2].contiguous(), track.rot[:K2].contiguous()
    short.rotvec, short.tcoef = track.rotvec[:K2 - 1].contiguous(), track.tcoef[:K2 - 1].contiguous()
    short.K = K2
    return short


@pytest.mark.parametrize("K", [4, 50])
def test_direct_pairs_vs_reference_loop_scipy_and_get_event_rays(synth, K):
    from enerf_amd.event_sampler import event_single_pair_rays
    from enerf_amd.events import get_event_rays
    ev, g, tables = synth
    num, first = g["xy_numEvs_Idx"][:, 0], g["xy_numEvs_Idx"][:, 1]
    P = len(num)
    track, slerp, cubic, _ = _scipy_track(K, float(ev[:, 2].min()), float(ev[:, 2].max()), 5 + K)
    two = np.nonzero(num == 2)[0]
    two = two[two > 0]
    assert len(two) >= 2, "the case needs pixels with exactly two events"
    rng = np.random.default_rng(K)
    for M in (1, 255, 257, P + 7):
        u = rng.random(P)
        choice = rng.integers(0, P, M) if M > P else rng.permutation(P)[:M]
        # the edges of the truncation on pixels that are chosen: the largest u below 1 (the pixel's last event with a
        # successor), u = 0 (-1: the event before the pixel's first, as the reference has it; not on pixel 0, where that is
        # no event), the smallest u above 0, and both edges on pixels with exactly two events
        TOP = 1.0 - 2.0 ** -53
        if M == 1:
            choice[0] = two[0]
            u[two[0]] = TOP if K == 4 else 0.0
        else:
            choice[:2] = two[:2]
            u[two[0]], u[two[1]] = TOP, 0.0
            rest = [int(c) for c in choice[2:] if c > 0 and c not in two[:2]]
            u[rest[0]], u[rest[1]], u[rest[2]], u[rest[3]] = 0.0, 0.0, TOP, 2.0 ** -53
        rs, re_, rp, rx, ry = EC.collate_single(g, u, choice)
        assert rs.min() >= 0
        out = event_single_pair_rays(tables, track, INTR_S, M, draws={"u_xy": torch.from_numpy(u),
                                                                      "choice": torch.from_numpy(choice)})
        assert np.array_equal(out["start"].cpu().numpy(), rs) and np.array_equal(out["end"].cpu().numpy(), re_)
        assert np.array_equal(out["pols"][0].cpu().numpy(), rp)
        assert int(out["outside_track"]) == 0 and int(out["bad_choice"]) == 0
        top, zero = u[choice] == TOP, u[choice] == 0.0
        assert top.any() or zero.any()
        assert np.array_equal(rs[top], (first + num - 2)[choice][top])            # the last event that has a successor
        assert np.array_equal(rs[zero], first[choice][zero] - 1)
        ref = get_event_rays(torch.from_numpy(rx)[None], torch.from_numpy(ry)[None],
                             _host_pose(slerp, cubic, g["events"][rs, 2]), _host_pose(slerp, cubic, g["events"][re_, 2]),
                             INTR_S)
        for k in RAYS:
            assert out[k].shape == (1, M, 3)
            np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].numpy(), rtol=0, atol=ATOL, err_msg=f"{k} M={M}")


def test_direct_pairs_own_draws_are_distinct_pixels_until_there_are_too_few(synth):
    from enerf_amd.event_sampler import event_single_pair_rays
    _, g, tables = synth
    P = len(g["xy_numEvs_Idx"])
    track, *_ = _scipy_track(50, 0.0, 1.5e7, 3)
    gen = torch.Generator(device=DEV).manual_seed(2)
    first = tables["first_at_xy"]
    evg = tables["events"]
    for M in (257, P, P + 7):
        r = event_single_pair_rays(tables, track, INTR_S, M, generator=gen)
        s, e = r["start"], r["end"]
        assert torch.equal(e, s + 1) and torch.equal(evg[s, :2], evg[e, :2]) and bool((evg[s, 2] < evg[e, 2]).all())
        assert torch.equal(r["pols"][0], evg[e, 3]) and int(r["bad_choice"]) == 0 and int(r["outside_track"]) == 0
        pixels = torch.searchsorted(first, s, right=True) - 1
        assert len(set(pixels.tolist())) == M if M <= P else len(set(pixels.tolist())) < M


# ------------------------------------------------------------------------------------------------ 3. synthetic, no events
@pytest.fixture(scope="module")
def noev():
    """Three 19 ms chunks of event-free pixels on 40 x 30 (rectified coordinates), a track reaching 5 ms past both ends."""
    from test_event_sampler import _no_event_case
    from enerf_amd.event_sampler import build_no_event_tables
    ev, rect, W, H, t0, t1 = _no_event_case(5)
    tab = build_no_event_tables(torch.from_numpy(ev).to(DEV), H, W, t0, t1, rectify_map=rect,
                                generator=torch.Generator(device=DEV).manual_seed(1))
    assert tab["N_ev_chunks"] == 3
    ref_tab = {"coords": [c.cpu().numpy() for c in tab["coords"]],
               "tss_bds": {"start_time_us": tab["start_time_us"], "end_time_us": tab["end_time_us"]}}
    return tab, ref_tab, _scipy_track(50, t0 * 1e3 - 5e6, t1 * 1e3 + 5e6, 8)


def _noev_draws(n, n_coords, seed):
    rng = np.random.default_rng(seed)
    idx, u = rng.integers(0, n_coords, n), rng.random((n, 2))
    u[0, 1] = 0.0                                                      # the chunk's first instant, and u[0, 0] > u[0, 1]
    if n > 1:
        u[1] = (0.75, 0.25)
        u[2] = (0.0, 0.0)
        idx[:2] = (0, n_coords - 1)
        assert (u[:, 0] > u[:, 1]).sum() > n // 4 and (u[:, 0] < u[:, 1]).sum() > n // 4
    return idx, u


@pytest.mark.parametrize("n", [1, 257])
def test_no_event_rays_vs_reference_loop_with_scipy_poses(noev, n):
    from enerf_amd.event_sampler import no_event_pair_rays
    from enerf_amd.events import get_event_rays
    tab, ref_tab, (track, slerp, cubic, _) = noev
    for chunk in (0, 2):
        idx, u = _noev_draws(n, len(ref_tab["coords"][chunk]), 11 + chunk)
        ref, tss = EC.no_event_rays(ref_tab, slerp, cubic, get_event_rays, INTR_S, 2 * n, chunk, idx, u)
        got = no_event_pair_rays(tab, track, INTR_S, 2 * n + 1, draws={"chunk": chunk, "idx": torch.from_numpy(idx),
                                                                      "u": torch.from_numpy(u)})
        assert got["tss_us"].dtype == torch.float64 and np.array_equal(got["tss_us"].cpu().numpy(), tss)
        assert int(got["outside_track"]) == 0 and int(got["bad_index"]) == 0
        for a, b in zip(NO_RAYS, RAYS):
            assert got[a].shape == (1, n, 3)
            np.testing.assert_allclose(got[a].cpu().numpy(), ref[b].numpy(), rtol=0, atol=ATOL, err_msg=f"{a} n={n}")
    own = no_event_pair_rays(tab, track, INTR_S, 2 * n, generator=torch.Generator(device=DEV).manual_seed(n))
    lo, hi = tab["start_time_us"][own["chunk"]], tab["end_time_us"][own["chunk"]]
    tss = own["tss_us"].cpu()
    assert bool((tss[:, 0] <= tss[:, 1]).all()) and float(tss.min()) >= lo and float(tss.max()) <= hi
    assert int(own["bad_index"]) == 0 and int(own["outside_track"]) == 0


# ------------------------------------------------------------------------------------------------ 4. the counters
def test_times_outside_the_track_are_counted_and_the_rest_is_unchanged(synth, noev):
    from enerf_amd.event_sampler import event_single_pair_rays, no_event_pair_rays
    ev, g, tables = synth
    P, M = len(g["xy_numEvs_Idx"]), 257
    track, _, _, knots = _scipy_track(50, float(ev[:, 2].min()), float(ev[:, 2].max()), 5)
    rng = np.random.default_rng(3)
    draws = {"u_xy": torch.from_numpy(rng.random(P)), "choice": torch.from_numpy(rng.permutation(P)[:M])}
    full = event_single_pair_rays(tables, track, INTR_S, M, draws=draws)
    half = event_single_pair_rays(tables, _cut(track, 25), INTR_S, M, draws=draws)
    t = tables["events"][:, 2].double()
    inside = ((t[full["start"]] <= float(knots[24])) & (t[full["end"]] <= float(knots[24]))).cpu()
    assert 0 < int(inside.sum()) < M
    assert int(full["outside_track"]) == 0 and int(half["outside_track"]) == M - int(inside.sum())
    assert torch.equal(half["start"], full["start"]) and torch.equal(half["pols"], full["pols"])
    for k in RAYS:
        assert torch.equal(half[k][0].cpu()[inside], full[k][0].cpu()[inside]), k
    # the no-event rays: the second half of the last chunk lies past a track cut in the middle
    tab, _, (ntrack, _, _, nknots) = noev
    n = 257
    idx, u = _noev_draws(n, tab["coords"][2].shape[0], 4)
    nd = {"chunk": 2, "idx": torch.from_numpy(idx), "u": torch.from_numpy(u)}
    nfull = no_event_pair_rays(tab, ntrack, INTR_S, 2 * n, draws=nd)
    K2 = int(np.searchsorted(nknots, 0.5 * (tab["start_time_us"][2] + tab["end_time_us"][2]) * 1e3))
    nhalf = no_event_pair_rays(tab, _cut(ntrack, K2), INTR_S, 2 * n, draws=nd)
    ninside = (nfull["tss_us"][:, 1] * 1000 <= float(nknots[K2 - 1])).cpu()
    assert 0 < int(ninside.sum()) < n
    assert int(nfull["outside_track"]) == 0 and int(nhalf["outside_track"]) == n - int(ninside.sum())
    assert torch.equal(nhalf["tss_us"], nfull["tss_us"])
    for k in NO_RAYS:
        assert torch.equal(nhalf[k][0].cpu()[ninside], nfull[k][0].cpu()[ninside]), k


def test_indices_that_are_none_are_counted_and_read_nothing(synth, noev):
    """Argument checks: the kernels compare every index with the table's length before they use it."""
    from enerf_amd.event_sampler import event_single_pair_rays, no_event_pair_rays
    ev, g, tables = synth
    P, M = len(g["xy_numEvs_Idx"]), 257
    track, *_ = _scipy_track(50, float(ev[:, 2].min()), float(ev[:, 2].max()), 5)
    rng = np.random.default_rng(6)
    u, choice = torch.from_numpy(rng.random(P)), torch.from_numpy(rng.permutation(P)[:M])
    good = event_single_pair_rays(tables, track, INTR_S, M, draws={"u_xy": u, "choice": choice})
    broken = choice.clone()
    broken[7], broken[256] = -1, P
    bad = event_single_pair_rays(tables, track, INTR_S, M, draws={"u_xy": u, "choice": broken})
    assert int(good["bad_choice"]) == 0 and int(bad["bad_choice"]) == 2 and int(bad["outside_track"]) == 0
    rows = torch.ones(M, dtype=torch.bool)
    rows[[7, 256]] = False
    for k in RAYS + ("pols",):
        assert torch.equal(bad[k][0].cpu()[rows], good[k][0].cpu()[rows]), k
        assert float(bad[k][0].cpu()[~rows].abs().sum()) == 0, k
    for k in ("start", "end"):
        assert torch.equal(bad[k].cpu()[rows], good[k].cpu()[rows]) and int(bad[k].cpu()[~rows].abs().sum()) == 0
    tab, _, (ntrack, *_) = noev
    n, n_coords = 257, tab["coords"][0].shape[0]
    idx, uu = _noev_draws(n, n_coords, 9)
    nd = {"chunk": 0, "idx": torch.from_numpy(idx), "u": torch.from_numpy(uu)}
    ngood = no_event_pair_rays(tab, ntrack, INTR_S, 2 * n, draws=nd)
    idx_b = idx.copy()
    idx_b[7], idx_b[256] = -1, n_coords
    nbad = no_event_pair_rays(tab, ntrack, INTR_S, 2 * n, draws=dict(nd, idx=torch.from_numpy(idx_b)))
    assert int(ngood["bad_index"]) == 0 and int(nbad["bad_index"]) == 2 and int(nbad["outside_track"]) == 0
    for k in NO_RAYS:
        assert torch.equal(nbad[k][0].cpu()[rows], ngood[k][0].cpu()[rows]), k
        assert float(nbad[k][0].cpu()[~rows].abs().sum()) == 0, k
    assert torch.equal(nbad["tss_us"].cpu()[rows], ngood["tss_us"].cpu()[rows])
    assert float(nbad["tss_us"].cpu()[~rows].abs().sum()) == 0


def test_entry_points_reject_what_they_cannot_serve():
    from enerf_amd import _lib as L
    z64 = torch.zeros(8, dtype=torch.float64, device=DEV)
    p = z64.data_ptr()
    lib = L.lib()
    single = lambda N, P, M, K, ev=p: lib.enerf_event_single_pair_rays(  # noqa: E731
        ev, N, p, p, P, p, p, M, p, p, p, p, K, 1.0, 1.0, 0.0, 0.0, p, p, p, p, p, p, p, p, p, None)
    noev = lambda nc, n, K, c=p: lib.enerf_no_event_rays(  # noqa: E731
        c, nc, p, p, n, 0.0, 1.0, p, p, p, p, K, 1.0, 1.0, 0.0, 0.0, p, p, p, p, p, p, p, None)
    assert single(0, 0, 0, 0) == 0 and noev(0, 0, 0) == 0                # nothing to do: no launch, no complaint
    for args in ((1, 1, 1, 2), (2, 0, 1, 2), (2, 1, 1, 1), (2, 1, 1, 2, None)):
        assert single(*args) != 0 and b"event_single_pair_rays" in lib.enerf_last_error()
    for args in ((0, 1, 2), (1, 1, 1), (1, 1, 2, None)):
        assert noev(*args) != 0 and b"no_event_rays" in lib.enerf_last_error()


# ------------------------------------------------------------------------------------------------ 5. the sampler
def _samplers(synth, noev, M, accumulate_evs=0, frames=False):
    from enerf_amd.event_sampler import EventSampler
    from enerf_amd.frame_sampler import FrameSampler
    from enerf_amd.pose_interp import PoseTrack
    ev, _, tables = synth
    tab, _, _ = noev
    # one track over the events (0 .. 15 ms) and the no-event chunks (1.000 s .. 1.057 s), in nanoseconds
    t, R, p = _track(50, 0.0, 1.1e9, 5)
    out = []
    for dev in ("cpu", DEV):
        fs = None
        if frames:
            g = torch.Generator().manual_seed(1)
            fs = FrameSampler(torch.eye(4).repeat(2, 1, 1).to(dev), INTR_S, 30, 40,
                              images=torch.rand(2, 30, 40, 1, generator=g).to(dev), num_rays=64)
        no_evs = dict(tab, coords=[c.to(dev) for c in tab["coords"]])
        evs = [torch.from_numpy(ev).to(dev), tables if dev == DEV else torch.from_numpy(ev[::-1].copy())]
        out.append(EventSampler(evs, PoseTrack(t, R.as_matrix(), p, device=dev), INTR_S, M, accumulate_evs, 3,
                                no_events=[no_evs, no_evs], frames=fs, seed=7))
    return out


@pytest.mark.parametrize("accumulate_evs", [0, 1])
def test_sampler_on_the_device_equals_the_cpu_sampler(synth, noev, accumulate_evs):
    cpu, gpu = _samplers(synth, noev, 300, accumulate_evs, frames=True)
    P, N = cpu.tables[1]["num_at_xy"].shape[0], cpu.tables[1]["events"].shape[0]
    rng = np.random.default_rng(1)
    draws = {"u_xy": torch.from_numpy(rng.random(P)), "choice": torch.from_numpy(rng.permutation(P)[:300]),
             "start": torch.from_numpy(rng.integers(0, N, 300)), "u_end": torch.from_numpy(rng.random(300)),
             "chunk": 1, "idx": torch.from_numpy(rng.integers(0, cpu.no_events[1]["coords"][1].shape[0], 150)),
             "u": torch.from_numpy(rng.random((150, 2))), "inds": torch.from_numpy(rng.integers(0, 1200, 64))}
    a = cpu.batch([1], draws=draws)
    b = gpu.batch([1], draws={k: v.to(DEV) if torch.is_tensor(v) else v for k, v in draws.items()})
    assert set(a) <= set(b) and set(b) - set(a) == {"outside_track", "no_evs_outside_track", "no_evs_bad_index"} | (
        set() if accumulate_evs else {"bad_choice"})
    for k in ("start", "end", "pols", "tss_us", "inds", "images"):
        assert torch.equal(a[k], b[k].cpu()), k
    assert (int((a["end"] - a["start"]).max()) > 1) == bool(accumulate_evs)
    for k in RAYS + NO_RAYS + ("rays_o", "rays_d"):
        assert a[k].shape == b[k].shape and b[k].dtype == torch.float32
        np.testing.assert_allclose(b[k].cpu().numpy(), a[k].numpy(), rtol=0, atol=ATOL, err_msg=k)
    assert a["chunk"] == b["chunk"] == 1 and a["index"] == b["index"] == [1] and (b["H"], b["W"]) == (30, 40)
    for k in set(b) - set(a):
        assert int(b[k]) == 0, k


def test_sampler_batch_waits_for_nothing_on_the_device(synth, noev):
    _, gpu = _samplers(synth, noev, 300, frames=True)
    gpu.batch([0])                                                     # (the library and the packed tables are in place)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [gpu.batch([v]) for v in (0, 1, 0)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    evg = gpu.tables[0]["events"]
    for b in (batches[0], batches[2]):
        s, e = b["start"], b["end"]
        assert torch.equal(e, s + 1) and torch.equal(evg[s, :2], evg[e, :2])
        assert all(int(b[k]) == 0 for k in ("outside_track", "bad_choice", "no_evs_outside_track", "no_evs_bad_index"))
        assert b["rays_no_evs_o1"].shape == (1, 150, 3) and 0 <= b["chunk"] < 3
    assert not torch.equal(batches[0]["start"], batches[2]["start"])


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_three_event_steps_from_the_sampler_on_the_route_of_the_shipped_configs():
    """accumulate_evs = 0, --negative_event_sampling, cuda_ray off, event_only: the sampler's batch through
    TrainHarness.step_events -- four renders by the stratified sampler's native route, one backward, one optimizer step."""
    from enerf_amd import scene, stratified
    from enerf_amd.event_sampler import EventSampler, build_event_tables, build_no_event_tables
    from enerf_amd.events import EventOptions
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.pose_interp import PoseTrack
    from enerf_amd.trainer import TrainHarness
    M, K = 512, 8
    rng = np.random.default_rng(0)
    n = 6000                                                           # 60 ms of events in the middle 48 x 40 pixels
    ev = np.stack([rng.integers(296, 344, n), rng.integers(220, 260, n), np.sort(rng.uniform(1.0e9, 1.06e9, n)),
                   rng.choice([-1.0, 1.0], n)], 1)
    poses = np.stack([scene.pose(0.25 * k).numpy() for k in range(K)])             # the camera on its circle, 70 ms
    track = PoseTrack(np.linspace(0.995e9, 1.065e9, K), poses[:, :3, :3], poses[:, :3, 3], device=DEV)
    tables = build_event_tables(torch.from_numpy(ev).float().to(DEV))
    no_evs = build_no_event_tables(torch.from_numpy(ev).to(DEV), scene.H, scene.W, 1.0e6, 1.06e6,
                                   generator=torch.Generator(device=DEV).manual_seed(0))
    sampler = EventSampler([tables], track, scene.INTRINSICS, M, no_events=[no_evs], seed=0, H=scene.H, W=scene.W)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=1).to(DEV)
    h = TrainHarness(model, lr=1e-2)
    opt = EventOptions(event_only=True, out_dim_color=1, negative_event_sampling=True, use_luma=False,
                       render_kwargs={"num_steps": 64, "upsample_steps": 0})
    table0 = model.encoder.embeddings.detach().clone()
    mlp0 = [p.detach().clone() for p in model.sigma_net.parameters()]
    calls = stratified.stats["calls"]
    losses = []
    for _ in range(3):
        b = sampler.batch([0])
        assert b["rays_evs_o1"].shape == (1, M, 3) and b["rays_no_evs_d2"].shape == (1, M // 2, 3)
        assert b["images"].shape == (1, 0, 3)
        losses.append(float(h.step_events(b, opt)))
    print(f"\nlosses {losses}, native renders {stratified.stats['calls'] - calls}")
    assert np.isfinite(losses).all()
    assert int(b["outside_track"]) == 0 and int(b["bad_choice"]) == 0 and int(b["no_evs_outside_track"]) == 0
    assert not torch.equal(model.encoder.embeddings.detach(), table0)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(model.sigma_net.parameters(), mlp0))
    assert stratified.stats["calls"] == calls + 3 * 4                  # two event and two no-event renders a step, all native
