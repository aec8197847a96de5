"""Mesh export on the MI355X (csrc/mesh.hip, enerf_amd/mesh.py): the lattice kernel against the
CPU linspace, the native marching cubes against the torch statement on the same device field, the native field against
model.density, and TrainHarness.save_mesh end to end in both shipped regimes."""
import numpy as np
import pytest
import torch

from util import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cpu_lattice(lo, hi, R, x0, nx):
    X, Y, Z = (torch.linspace(lo[a], hi[a], R) for a in range(3))
    xx, yy, zz = torch.meshgrid(X[x0:x0 + nx], Y, Z, indexing="ij")
    return torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1)


@pytest.mark.parametrize("R", [2, 130, 256, 257])
def test_lattice_points_bit_equal_cpu_linspace(R):
    from enerf_amd import mesh
    for lo, hi in (([-1.0, -2.0, -4.0], [1.0, 2.0, 4.0]), ([-1.5, -3.25, -1.1], [3.7, 1.3, 2.9])):
        lo = [float(np.float32(v)) for v in lo]
        hi = [float(np.float32(v)) for v in hi]
        # slabs at both ends and across the midpoint (where linspace switches formula) and the reference's block edge
        for x0, nx in {(0, min(R, 3)), (max(0, R // 2 - 2), min(R - max(0, R // 2 - 2), 4)), (max(0, R - 3), min(R, 3)),
                       (min(126, R - 1), min(4, R - min(126, R - 1)))}:
            got = mesh.lattice_points(lo, hi, R, x0, nx, DEV).cpu()
            want = _cpu_lattice(lo, hi, R, x0, nx)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (R, lo, hi, x0, nx)


def _field(kind, R, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        u = torch.randn(R, R, R, generator=g)
        return u, float(u.median())
    if kind == "tied":
        u = torch.round(torch.randn(R, R, R, generator=g) * 2) / 2
        return u, 0.5
    if kind == "empty":
        return torch.full((R, R, R), -1.0), 0.0
    if kind == "full":
        return torch.full((R, R, R), 1.0), 0.0
    c = torch.tensor([0.37, 0.41, 0.33]) * (R - 1) + 0.13                  # analytic: a sphere off the lattice
    x = torch.stack(torch.meshgrid(*[torch.arange(R, dtype=torch.float64)] * 3, indexing="ij"), -1)
    return (0.3 * (R - 1) - (x - c.double()).norm(dim=-1)).float(), 0.0


@pytest.mark.parametrize("R", [2, 3, 17, 64, 130, 256])
@pytest.mark.parametrize("kind", ["random", "analytic", "tied", "empty", "full"])
def test_native_marching_cubes_equals_statement(R, kind):
    from enerf_amd import mesh
    u, thr = _field(kind, R, R)
    u = u.to(DEV)
    v, f = mesh.marching_cubes(u, thr)
    v_ref, f_ref = mesh.marching_cubes_statement(u, thr)
    assert v.is_cuda and v.dtype == torch.float64 and f.dtype == torch.int32
    assert torch.equal(v.view(torch.int64), v_ref.view(torch.int64)), (R, kind)
    assert torch.equal(f, f_ref), (R, kind)
    if kind in ("empty", "full"):
        assert v.shape == (0, 3) and f.shape == (0, 3)
    if kind == "analytic" and R >= 17:
        assert f.shape[0] > 0


def test_native_rejects_non_finite():
    from enerf_amd import mesh
    u = torch.randn(33, 33, 33, device=DEV)
    u[3, 4, 5], u[32, 32, 32], u[0, 0, 0] = float("nan"), float("inf"), -float("inf")
    with pytest.raises(ValueError, match="3 non-finite"):
        mesh.marching_cubes(u, 0.0)
    torch.cuda.synchronize()


def _model(seed=5, bound=2):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(seed)
    model = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), seed, -0.5, 0.5)
    return model.to(DEV).eval()


def _density_on_lattice(model, R, lo, hi):
    from enerf_amd import mesh
    out = torch.empty(R, R, R, device=DEV)
    for x0 in range(0, R, 16):
        n = min(16, R - x0)
        pts = mesh.lattice_points(lo, hi, R, x0, n, DEV)
        out[x0:x0 + n] = model.density(pts)["sigma"].float().view(n, R, R)
    return out


@pytest.mark.parametrize("R", [65, 160])
def test_field_fp32_against_model_density(R):
    """fp32: the sigma net's own kernels on the same points (model.density runs them through fused_mlp): sigma to the
    round-off the stratified tests allow the sigma net (1e-4 relative; sigma = exp(h0) passes h0's error on)."""
    from enerf_amd import mesh
    model = _model()
    lo, hi = [-2.0] * 3, [2.0] * 3
    with torch.no_grad():
        u = mesh.density_field(model, R, lo, hi)
        ref = _density_on_lattice(model, R, lo, hi)
    torch.testing.assert_close(u, ref, rtol=1e-4, atol=1e-6)
    assert "_density_scratch" not in model.__dict__


def test_field_precision3_against_autocast_statement():
    """Precision 3 (fp16 operands, fp32 accumulation) against model.density under autocast(fp16), the reference's
    query: both round the features and the hidden layer to fp16, in different places (autocast also rounds the output
    h0 before exp).  Bar: |log sigma| differences <= 2e-2 (about 10 fp16 ulps of h0 at |h0| ~ 1), median <= 2e-3."""
    from enerf_amd import mesh
    model = _model()
    R, lo, hi = 96, [-2.0] * 3, [2.0] * 3
    model.mlp_precision = 3
    try:
        with torch.no_grad():
            u = mesh.density_field(model, R, lo, hi)
    finally:
        del model.mlp_precision
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = _density_on_lattice(model, R, lo, hi)
        assert not mesh._field_supported(model, torch.device(DEV))
    d = (u.log() - ref.log()).abs()
    assert float(d.max()) <= 2e-2 and float(d.median()) <= 2e-3, (float(d.max()), float(d.median()))
    with torch.no_grad():
        u32 = mesh.density_field(model, R, lo, hi)
    assert not torch.equal(u, u32)                                   # (the regime did reach the kernels)


def _trained_harness(fp16):
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=False, out_dim_color=3).to(DEV)
    h = TrainHarness(model, lr=1e-2, fp16=fp16)
    assert h.strat_f16 == bool(fp16)
    g = np.random.default_rng(1)
    for i in range(6):
        v = g.normal(size=(1024, 3))
        o = 3.5 * v / np.linalg.norm(v, axis=1, keepdims=True)
        d = g.uniform(-1.5, 1.5, (1024, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)  # noqa: E731
        target = f(g.uniform(0, 1, (1024, 3)))
        h.step_rgb(f(o), f(d), target, num_steps=64, upsample_steps=0, out_dim_color=3)
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("fp16", [False, True])
def test_save_mesh_end_to_end(tmp_path, fp16):
    from enerf_amd import mesh
    h = _trained_harness(fp16)
    model = h.model
    R = 256
    box = model.aabb_infer.cpu().numpy()
    # the threshold: the field's median (a few steps in, sigma sits far from the reference's 10)
    prev = h._amp_scope() if fp16 else None
    try:
        u = mesh.density_field(model, R, box[:3], box[3:])
    finally:
        if fp16:
            h._amp_restore(prev)
    thr = float(u.median())
    v_ref, f_ref = mesh.marching_cubes_statement(u, thr)
    v_ref = mesh.to_world(v_ref, R, box[:3], box[3:])
    del u
    torch.cuda.synchronize()
    scratch = "_density_scratch" in model.__dict__
    before = torch.cuda.memory_allocated()
    v, f = h.save_mesh(str(tmp_path / "a.ply"), resolution=R, threshold=thr)
    torch.cuda.synchronize()
    assert f.shape[0] > 0
    assert torch.equal(f, f_ref) and torch.equal(v.view(torch.int64), v_ref.view(torch.int64))
    del v, f
    assert torch.cuda.memory_allocated() == before
    assert ("_density_scratch" in model.__dict__) == scratch
    assert model.__dict__.get("mlp_precision") is None
    h.save_mesh(str(tmp_path / "b.ply"), resolution=R, threshold=thr)
    a, b = open(tmp_path / "a.ply", "rb").read(), open(tmp_path / "b.ply", "rb").read()
    assert a == b
    rv, rf = mesh.read_ply(str(tmp_path / "a.ply"))
    assert len(rf) == len(f_ref) and (rv >= box[:3]).all() and (rv <= box[3:]).all()
