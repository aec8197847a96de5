"""Mesh export on the CPU (enerf_amd/mc_table.py, enerf_amd/mesh.py): the generated table, the
torch statement of marching cubes against a scalar oracle written here, analytic surfaces, the PLY writer, and the field
and world mapping against the reference's own extract_fields / extract_geometry (tests/golden/ref_mesh_field.npz, minted
by tests/refcheck/mint_mesh_golden.py)."""
import hashlib
import math
from collections import Counter

import numpy as np
import pytest
import torch

from util import golden, det_fill_


# ------------------------------------------------------------------------------------------------------------ table
def test_generated_header_is_committed():
    from enerf_amd import mc_table
    with open(mc_table.HEADER) as f:
        assert f.read() == mc_table.header_text()
    counts, edges, max_tri = mc_table.build_tables()
    assert max_tri == int(counts.max()) and edges.shape == (256, max_tri, 3)


def test_crossed_edges_per_case():
    from enerf_amd import mc_table as M
    for case in range(256):
        above = [(case >> k) & 1 for k in range(8)]
        want = set()
        for e in range(12):
            c0 = M.EDGE_CORNER[e]
            dx, dy, dz = M.CORNERS[c0]
            d = [0, 0, 0]
            d[M.EDGE_AXIS[e]] = 1
            c1 = M.CORNERS.index((dx + d[0], dy + d[1], dz + d[2]))
            if above[c0] != above[c1]:
                want.add(e)
        used = {e for t in M.case_triangles(case) for e in t}
        assert used == want, case
        assert (len(M.case_triangles(case)) == 0) == (case in (0, 255))


def test_triangle_edges_pair_up_inside_each_case():
    """Within a case, a triangle edge on a cube face is one of the face's segments (once); every other one appears twice,
    in opposite directions."""
    from enerf_amd import mc_table as M
    for case in range(256):
        segs = {s for f in M.FACES for s in M._face_segments(case, f)}
        seen = Counter()
        for a, b, c in M.case_triangles(case):
            for e in ((a, b), (b, c), (c, a)):
                seen[e] += 1
        for (a, b), n in seen.items():
            assert n == 1, (case, a, b)
            if (a, b) in segs:
                assert (b, a) not in seen, (case, a, b)
            else:
                assert seen[(b, a)] == 1, (case, a, b)
        assert {s for s in segs} <= set(seen), case


# ------------------------------------------------------------------------------------------ scalar oracle (per cell)
def oracle_mc(u, thr):
    """Per-point, per-cell loops with a dict of edges: the semantics of mesh.py written out once more."""
    from enerf_amd import mc_table as M
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    up = lambda v: float(v) > thr  # noqa: E731
    verts, index = [], {}
    for x in range(R):
        for y in range(R):
            for z in range(R):
                p = (x, y, z)
                for a in range(3):
                    q = list(p)
                    q[a] += 1
                    if q[a] >= R or up(u[p]) == up(u[tuple(q)]):
                        continue
                    u0, u1 = float(u[p]), float(u[tuple(q)])
                    v = [float(x), float(y), float(z)]
                    v[a] = v[a] + (thr - u0) / (u1 - u0)
                    index[(p, a)] = len(verts)
                    verts.append(v)
    tris = []
    for x in range(R - 1):
        for y in range(R - 1):
            for z in range(R - 1):
                case = 0
                for k, (dx, dy, dz) in enumerate(M.CORNERS):
                    case |= int(up(u[x + dx, y + dy, z + dz])) << k
                for t in M.case_triangles(case):
                    row = []
                    for e in t:
                        dx, dy, dz = M.CORNERS[M.EDGE_CORNER[e]]
                        row.append(index[((x + dx, y + dy, z + dz), M.EDGE_AXIS[e])])
                    tris.append(row)
    return np.array(verts, np.float64).reshape(-1, 3), np.array(tris, np.int32).reshape(-1, 3)


def _fields(R, seed):
    g = np.random.default_rng(seed)
    r = g.standard_normal((R, R, R)).astype(np.float32)
    out = [(r, float(np.quantile(r, q))) for q in (0.1, 0.5, 0.9)]
    tied = np.round(r * 2).astype(np.float32) / 2                        # many exact ties with 0 and 0.5
    out += [(tied, 0.0), (tied, 0.5)]
    out += [(np.full((R, R, R), 3.0, np.float32), 1.0), (np.full((R, R, R), -3.0, np.float32), 1.0)]
    out += [(np.full((R, R, R), 1.0, np.float32), 1.0)]                 # all equal to the threshold: all below
    return out


@pytest.mark.parametrize("R", [2, 3, 9, 17])
def test_statement_equals_scalar_oracle(R):
    from enerf_amd import mesh
    for i, (u, thr) in enumerate(_fields(R, 100 + R)):
        v, f = mesh.marching_cubes(torch.from_numpy(u), thr)
        v_ref, f_ref = oracle_mc(u, thr)
        assert v.dtype == torch.float64 and f.dtype == torch.int32, i
        assert np.array_equal(v.numpy().view(np.uint64), v_ref.view(np.uint64)), (R, i)
        assert np.array_equal(f.numpy(), f_ref), (R, i)


def test_resolution_and_field_checks():
    from enerf_amd import mesh
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(1, 1, 1), 0.0)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(2, 3, 2), 0.0)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(2, 2, 2, dtype=torch.float64), 0.0)
    u = torch.zeros(5, 5, 5)
    u[1, 2, 3], u[4, 4, 4], u[0, 0, 0] = float("nan"), float("inf"), -float("inf")
    with pytest.raises(ValueError, match="3 non-finite"):
        mesh.marching_cubes(u, 0.0)


# ------------------------------------------------------------------------------------------------ analytic surfaces
def _mesh_topology(v, f):
    """-> (closed 2-manifold with consistent orientation, Euler characteristic, signed volume)."""
    F = f.astype(np.int64)
    directed = Counter()
    for t in F:
        for i in range(3):
            directed[(t[i], t[(i + 1) % 3])] += 1
    ok = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    used = np.unique(F)
    euler = len(used) - len(directed) // 2 + len(F)
    a, b, c = v[F[:, 0]], v[F[:, 1]], v[F[:, 2]]
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)
    return ok, euler, vol


def sphere_field(R, c, r):
    g = np.stack(np.meshgrid(*[np.arange(R, dtype=np.float64)] * 3, indexing="ij"), -1)
    return (r - np.linalg.norm(g - np.asarray(c), axis=-1)).astype(np.float32)


def test_sphere():
    from enerf_amd import mesh
    h, r, R = 1.0, 20.0, 48
    c = (23.31, 23.77, 22.58)                          # off the lattice
    v, f = mesh.marching_cubes(torch.from_numpy(sphere_field(R, c, r)), 0.0)
    v, f = v.numpy(), f.numpy()
    d = np.abs(np.linalg.norm(v - np.asarray(c), axis=1) - r)
    assert d.max() <= h * h / (8 * (r - h)) + 1e-6, d.max()
    ok, euler, vol = _mesh_topology(v, f)
    assert ok and euler == 2
    want = 4 / 3 * math.pi * r ** 3
    assert vol > 0 and abs(vol - want) / want < 0.01, (vol, want)


def test_torus():
    from enerf_amd import mesh
    R, big, small = 56, 16.0, 6.0
    c = np.array([27.4, 27.9, 27.2])
    g = np.stack(np.meshgrid(*[np.arange(R, dtype=np.float64)] * 3, indexing="ij"), -1) - c
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - big
    u = (small - np.sqrt(q ** 2 + g[..., 2] ** 2)).astype(np.float32)
    v, f = mesh.marching_cubes(torch.from_numpy(u), 0.0)
    ok, euler, vol = _mesh_topology(v.numpy(), f.numpy())
    want = 2 * math.pi ** 2 * big * small ** 2
    assert ok and euler == 0
    assert vol > 0 and abs(vol - want) / want < 0.02, (vol, want)


# ------------------------------------------------------------------------------------------------------------- PLY
def test_ply_round_trip(tmp_path):
    from enerf_amd import mesh
    g = np.random.default_rng(3)
    v = g.uniform(-2, 2, (50, 3))
    f = g.integers(0, 50, (70, 3)).astype(np.int32)
    p = mesh.write_ply(str(tmp_path / "m.ply"), torch.from_numpy(v), torch.from_numpy(f))
    data = open(p, "rb").read()
    assert data.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 50\n")
    assert b"property list uchar int vertex_indices\nend_header\n" in data
    rv, rf = mesh.read_ply(p)
    assert np.array_equal(rv, v.astype(np.float32)) and np.array_equal(rf, f)
    # an independent parse of the body: 12 bytes per vertex, then 13 per face
    body = data[data.index(b"end_header\n") + 11:]
    assert len(body) == 50 * 12 + 70 * 13
    assert np.frombuffer(body[:600], "<f4").reshape(50, 3).tolist() == v.astype(np.float32).tolist()
    assert body[600] == 3 and np.frombuffer(body[601:613], "<i4").tolist() == f[0].tolist()


def test_ply_empty_mesh(tmp_path):
    from enerf_amd import mesh
    p = mesh.write_ply(str(tmp_path / "e.ply"), torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.int32))
    rv, rf = mesh.read_ply(p)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    assert b"element vertex 0\n" in open(p, "rb").read()


def test_no_mcubes_or_trimesh_imported():
    import subprocess
    import sys
    code = ("import sys, enerf_amd.mesh, enerf_amd.trainer; "
            "assert 'mcubes' not in sys.modules and 'trimesh' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code])


# ------------------------------------------------------------------------------------------- against the reference
def _golden_model(g):
    from enerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=int(g["bound"]), cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), int(g["seed"]), float(g["fill_lo"]), float(g["fill_hi"]))
    return model.eval()


def test_density_field_equals_reference_extract_fields(cpu_oracle_backend):
    """R = 130 crosses the reference's 128^3 block on every axis; the field must be its field, bit for bit."""
    from enerf_amd import mesh
    g = golden("ref_mesh_field")
    model = _golden_model(g)
    box = model.aabb_infer.numpy()
    assert np.array_equal(box, g["aabb"])
    R = int(g["resolution"])
    u = mesh.density_field(model, R, box[:3], box[3:]).numpy()
    assert u.shape == (R, R, R) and u.dtype == np.float32
    pl = list(g["planes"])
    assert np.array_equal(u[pl].view(np.uint32), g["u_x"].view(np.uint32))
    assert np.array_equal(u[:, pl].view(np.uint32), g["u_y"].view(np.uint32))
    assert np.array_equal(u[:, :, pl].view(np.uint32), g["u_z"].view(np.uint32))
    assert hashlib.sha256(u.tobytes()).digest() == g["sha256"].tobytes()
    assert "_density_scratch" not in model.__dict__


def test_world_mapping_equals_reference_extract_geometry():
    from enerf_amd import mesh
    g = golden("ref_mesh_field")
    box = g["aabb"]
    w = mesh.to_world(torch.from_numpy(g["stub_vertices"]), int(g["resolution"]), box[:3], box[3:])
    assert w.dtype == torch.float64
    assert np.array_equal(w.numpy().view(np.uint64), g["world_vertices"].view(np.uint64))


def test_harness_save_mesh_cpu(tmp_path, cpu_oracle_backend):
    """The public entry point on a CPU model: the reference's blocks, the statement, a PLY whose vertices are the
    returned ones rounded to fp32."""
    from enerf_amd import mesh
    from enerf_amd.network import NeRFNetwork
    from enerf_amd.trainer import TrainHarness
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), 5, -0.5, 0.5)
    h = TrainHarness(model)
    u = mesh.density_field(model, 24, [-1.0] * 3, [1.0] * 3)
    thr = float(u.median())
    v, f = h.save_mesh(str(tmp_path / "sub" / "mesh.ply"), resolution=24, threshold=thr)
    v2, f2 = mesh.marching_cubes_statement(u, thr)
    assert torch.equal(f, f2) and torch.equal(v, mesh.to_world(v2, 24, [-1.0] * 3, [1.0] * 3))
    rv, rf = mesh.read_ply(str(tmp_path / "sub" / "mesh.ply"))
    assert len(rf) > 0 and np.array_equal(rf, f.numpy()) and np.array_equal(rv, v.numpy().astype(np.float32))
    assert (rv >= -1).all() and (rv <= 1).all()
