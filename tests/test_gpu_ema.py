"""The parameters' exponential moving average on the MI355X (csrc/optim.hip k_ema_multi, enerf_amd/ema.py; DESIGN.md
section 4.14): the kernel against the torch statement on the same device, its bounds, the split over 16 tensors, the
checkpoint round trip, and a harness that evaluates with its average in the middle of training against twins that do not.

Launch geometry the sizes below come from (enerf_ema_update_multi): blocks of 256 threads, at most 2048 blocks per tensor;
a tensor whose two pointers are 16-byte aligned is walked as float4 (a block's share of one pass: 1024 floats, the grid's:
2048 * 1024), any other element by element (256 and 2048 * 256)."""
import argparse as ap
import ctypes

import pytest
import torch

from util import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8                       # floats in front of and behind every buffer (32 bytes: the view stays 16-byte aligned)
SENTINEL = 0x7F4D5A11           # (a NaN's bits: arithmetic on a guard word would not leave it unchanged either)
BLOCK_VEC, GRID_VEC = 1024, 2048 * 1024
BLOCK_SCALAR, GRID_SCALAR = 256, 2048 * 256


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)               # (any dtype)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _same(a, b):
    """Bit for bit, a NaN for a NaN (which NaN an operation on NaNs hands on is the instruction's choice, not the sum's)."""
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _guarded(n, offset, gen, special=True):
    """-> (buffer, view of n floats starting `offset` floats past the 16-byte aligned start), guard words around it."""
    buf = torch.empty(GUARD + offset + n + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_((torch.rand(n, device=DEV, generator=gen) - 0.5) * 4)
    if special and n >= 16:
        view[5:12] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-41, -1e-41, 3e38], device=DEV)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def _guards_intact(buf, offset, n):
    w = buf.view(torch.int32)
    return bool((w[:GUARD + offset] == SENTINEL).all()) and bool((w[GUARD + offset + n:] == SENTINEL).all())


def _call(shadows, params, omd):
    from enerf_amd import _lib as L
    n = len(shadows)
    vp, sz = ctypes.c_void_p * n, ctypes.c_size_t * n
    return L.lib().enerf_ema_update_multi(n, vp(*[t.data_ptr() for t in shadows]), vp(*[t.data_ptr() for t in params]),
                                          sz(*[t.numel() for t in shadows]), omd, L.stream_handle())


# (n, offset of the shadow, offset of the parameter) per tensor of one call
SINGLE = [[(n, 0, 0)] for n in (1, 3, 4, 5, 1023, 1024, 1025)]
CASES = SINGLE + [
    [(3 * BLOCK_VEC + 5, 0, 0)],                         # more than one block's share
    [(GRID_VEC + BLOCK_VEC + 3, 0, 0)],                  # more than one pass of the whole grid
    [(1029, 1, 0)], [(1029, 0, 1)], [(1030, 1, 1)], [(7, 3, 2)],             # the element-by-element path
    [(3 * BLOCK_SCALAR + 1, 1, 0)], [(GRID_SCALAR + BLOCK_SCALAR + 77, 1, 3)],
    [(1025, 0, 0), (0, 0, 0)],
    [(0, 0, 0), (1023, 1, 0)],
    [(1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 1, 0), (1023, 0, 0), (1024, 0, 0), (1025, 0, 2), (0, 0, 0),
     (3 * BLOCK_VEC + 5, 0, 0), (GRID_VEC + BLOCK_VEC + 3, 0, 0), (3 * BLOCK_SCALAR + 1, 1, 0), (0, 0, 0),
     (GRID_SCALAR + BLOCK_SCALAR + 77, 3, 0), (2, 0, 0), (6, 2, 2), (4099, 0, 0)],
]


def _case_id(case):
    return f"{len(case)}x" + "_".join(f"{n}+{a}+{b}" for n, a, b in case[:3])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_against_the_statement(case):
    from enerf_amd.ema import ema_statement
    assert len(case) in (1, 2, 16)
    gen = torch.Generator(device=DEV).manual_seed(len(case) * 1000 + case[0][0])
    sb = [_guarded(n, a, gen) for n, a, _ in case]
    pb = [_guarded(n, b, gen) for n, _, b in case]
    shadows, params = [v for _, v in sb], [v for _, v in pb]
    kept = [p.clone() for p in params]
    for omd in (1.0 - 2.0 / 11.0, 1.0 - 0.95):           # (two updates in a row: the second reads what the first wrote)
        want = [ema_statement(s.clone(), p, omd) for s, p in zip(shadows, params)]
        assert _call(shadows, params, omd) == 0
        torch.cuda.synchronize()
        for k, (s, w) in enumerate(zip(shadows, want)):
            assert _same(s, w), (k, case[k])
    for (buf, _), (n, a, _) in zip(sb, case):
        assert _guards_intact(buf, a, n)
    for (buf, _), (n, _, b), p, q in zip(pb, case, params, kept):
        assert _guards_intact(buf, b, n) and _same_bits(p, q)            # the parameters are only read


def test_bad_arguments_and_empty_calls():
    from enerf_amd import _lib as L
    gen = torch.Generator(device=DEV).manual_seed(1)
    s = [_guarded(8, 0, gen, special=False)[1] for _ in range(17)]
    p = [_guarded(8, 0, gen, special=False)[1] for _ in range(17)]
    kept = [t.clone() for t in s]
    assert _call(s, p, 0.5) == -1                                           # ENERF_E_BADARG: count > 16
    assert b"16" in L.lib().enerf_last_error()
    vp, sz = ctypes.c_void_p * 1, ctypes.c_size_t * 1
    assert L.lib().enerf_ema_update_multi(1, vp(None), vp(p[0].data_ptr()), sz(8), 0.5, L.stream_handle()) == -1
    assert L.lib().enerf_ema_update_multi(1, vp(s[0].data_ptr()), vp(None), sz(8), 0.5, L.stream_handle()) == -1
    assert L.lib().enerf_ema_update_multi(1, vp(None), vp(None), sz(0), 0.5, L.stream_handle()) == 0     # n = 0: a no-op
    assert L.lib().enerf_ema_update_multi(0, None, None, None, 0.5, L.stream_handle()) == 0
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(s, kept))


def test_update_over_17_tensors_is_two_launches(monkeypatch):
    from enerf_amd import _lib as L
    from enerf_amd.ema import ParamEMA, ema_statement
    gen = torch.Generator(device=DEV).manual_seed(17)
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, 2, 7, 64, 255, 256, 257, 4099, 12, 31, 33]
    params = [torch.nn.Parameter((torch.rand(n, device=DEV, generator=gen) - 0.5) * 4) for n in sizes]
    half = torch.nn.Parameter(torch.rand(9, device=DEV, generator=gen).half())           # takes the statement
    strided = torch.nn.Parameter(torch.rand(6, 4, device=DEV, generator=gen).t())         # so does this one
    assert not strided.is_contiguous()
    ema = ParamEMA(params + [half, strided], 0.95)
    want = [p.detach().clone() for p in ema.parameters]
    with torch.no_grad():
        for p in ema.parameters:
            p.add_(0.25)
    lib = L.lib()
    counts = []
    raw = lib.enerf_ema_update_multi

    def spy(count, *a):
        counts.append(int(count))
        return raw(count, *a)
    monkeypatch.setattr(lib, "enerf_ema_update_multi", spy)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ema.update()
    assert torch.cuda.memory_allocated() == before                       # nothing allocated that stays
    assert counts == [16, 1]
    monkeypatch.undo()
    for w, p in zip(want, ema.parameters):
        ema_statement(w, p.detach(), 1.0 - 2.0 / 11.0)
    torch.cuda.synchronize()
    assert ema.num_updates == 1
    assert all(_same_bits(s, w) for s, w in zip(ema.shadow_params, want))


# ------------------------------------------------------------------------------------------------------ the harness
def _harness(seed=7, ema_decay=None, fill=True):
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, out_dim_color=3)
    if fill:
        det_fill_(list(model.parameters()), seed, -0.25, 0.25)
    model = model.to(DEV)
    return model, TrainHarness(model, lr=1e-2, occupancy="synthetic", ema_decay=ema_decay)


def test_checkpoint_round_trip(tmp_path):
    from test_gpu_training import _batches
    data = _batches(2, 1024, 2)
    model, h = _harness(ema_decay=0.95)
    for k in range(2):
        h.step_rgb(*data[k])
        h.ema.update()
    path = h.save_checkpoint(str(tmp_path / "ngp_ep0001.pth"), full=True)
    f = torch.load(path, map_location="cpu", weights_only=True)
    assert set(f["ema"]) == {"decay", "num_updates", "shadow_params", "collected_params"}
    for model_only in (True, False):
        model2, h2 = _harness(seed=9, ema_decay=0.5, fill=False)
        assert not _same_bits(h2.ema.shadow_params[0], h.ema.shadow_params[0])
        h2.load_checkpoint(path if model_only else f, model_only=model_only)      # (the file once, then its dict)
        assert h2.ema.decay == 0.95 and h2.ema.num_updates == 2
        assert all(s.device == p.device and s.dtype == p.dtype and _same_bits(s, t)
                   for s, p, t in zip(h2.ema.shadow_params, model2.parameters(), h.ema.shadow_params))
        assert h2.global_step == (0 if model_only else 2)
        # the loaded average moves on like the one that was saved
        h2.ema.update(list(model.parameters()))
        twin = [s.clone() for s in h.ema.shadow_params]
        from enerf_amd.ema import ema_statement
        for s, p in zip(twin, model.parameters()):
            ema_statement(s, p.detach(), 1.0 - 4.0 / 13.0)
        assert h2.ema.num_updates == 3 and all(_same_bits(a, b) for a, b in zip(h2.ema.shadow_params, twin))
    # a file without the key leaves the average as it is; a harness without an average ignores the key
    kept = [s.clone() for s in h2.ema.shadow_params]
    h2.load_checkpoint({k: v for k, v in f.items() if k != "ema"})
    assert h2.ema.num_updates == 3 and all(_same_bits(a, b) for a, b in zip(h2.ema.shadow_params, kept))
    _, plain = _harness(seed=10, fill=False)
    plain.load_checkpoint(f)
    assert plain.ema is None and plain.global_step == 2


def _views(V=2, side=16, seed=21):
    from enerf_amd import scene
    j, i = torch.meshgrid(torch.arange(side, device=DEV) * (scene.H // side),
                          torch.arange(side, device=DEV) * (scene.W // side), indexing="ij")
    inds = (j * scene.W + i).reshape(-1)
    g = torch.Generator().manual_seed(seed)
    views = []
    for k in range(V):
        ro, rd = scene.pixel_rays(scene.pose(5 * k + 2), inds, DEV)
        views.append({"rays_o": ro, "rays_d": rd, "images": torch.rand(1, side, side, 3, generator=g), "H": side,
                      "W": side})
    return views


def test_harness_with_an_average_and_twins_without():
    """Three steps, then the first harness updates its average and evaluates with it, then one more step for everybody.
    The twins (same fill, same rays, no average) are the yardstick of the fourth step: the step's coarse-level
    gradients are float atomic sums, so two runs of the same training need not agree to the bit, and the bound on
    |loss - twin's loss| is the spread measured among the twins themselves (four of them: their largest pairwise
    difference, zero if the step is deterministic), taken to the nearest twin."""
    from test_gpu_training import _batches
    data = _batches(4, 1024, 2)
    opt = ap.Namespace(event_only=False, out_dim_color=3, color_space="srgb", render_kwargs={})
    views = _views()
    model, h = _harness(ema_decay=0.95)
    twins = [_harness() for _ in range(4)]
    assert all(t.ema is None for _, t in twins)
    for k in range(3):
        h.step_rgb(*data[k])
        for _, t in twins:
            t.step_rgb(*data[k])
    assert h._native_route_sig is not None and all(t._native_route_sig is not None for _, t in twins)   # the one-call step
    h.ema.update()
    assert not _same_bits(h.ema.shadow_params[0], model.encoder.embeddings)
    before = [p.detach().clone() for p in model.parameters()]
    ptrs = [p.data_ptr() for p in model.parameters()]
    r = h.evaluate(views, opt)
    assert all(_same_bits(p, b) for p, b in zip(model.parameters(), before))
    assert [p.data_ptr() for p in model.parameters()] == ptrs and model.training
    # a third model whose parameters ARE the average, evaluated twice: the spread of the render itself
    model3, h3 = _harness()
    with torch.no_grad():
        for p, s in zip(model3.parameters(), h.ema.shadow_params):
            p.copy_(s)
    a, b = h3.evaluate(views, opt)["valid_loss"], h3.evaluate(views, opt)["valid_loss"]
    print(f"valid_loss: ema {r['valid_loss']!r}, third model {a!r} / {b!r}")
    assert abs(r["valid_loss"] - a) <= abs(a - b)
    # the fourth step: nothing of the swapped-in weights survives
    mine = float(h.step_rgb(*data[3]))
    theirs = [float(t.step_rgb(*data[3])) for _, t in twins]
    spread = max(theirs) - min(theirs)
    print(f"fourth step: {mine!r} against twins {theirs!r} (spread {spread!r})")
    assert min(abs(mine - t) for t in theirs) <= spread
    own = twins[0][1].evaluate(views, opt)["valid_loss"]                  # (trained weights give another number)
    assert abs(own - a) > abs(a - b), (own, a, b)
