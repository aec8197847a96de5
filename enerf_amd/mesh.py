"""Mesh export: the density lattice and marching cubes of the reference's `Trainer.save_mesh` (nerf/utils.py:219-249,
712-732), with the hot path in HIP (csrc/mesh.hip) and no PyMCubes / trimesh.

    density_field(model, R, lo, hi)     sigma on the R^3 lattice of torch.linspace(lo, hi, R) per axis -> u [R, R, R] fp32
    marching_cubes(u, threshold)        -> vertices [V, 3] fp64 (index space), triangles [F, 3] int32
    extract_geometry(model, R, thr)     the two over model.aabb_infer, vertices mapped to world coordinates
    write_ply(path, vertices, triangles)

Semantics, the same on every path:
  * u[x, y, z], x slowest; lattice coordinate i of an axis = torch.linspace(lo, hi, R)[i] as the CPU computes it.
  * A corner is above when u > threshold (compared in fp64).  An edge whose ends differ is crossed and carries one vertex,
    owned by its lower-index end: p + t e_axis, t = (threshold - u[p]) / (u[p + e] - u[p]) in fp64.  Vertices are ordered
    by the owner's linear index, then by axis.
  * Triangles: by cell linear index (x slowest), then in the order of the cell's case in csrc/mc_tables.h
    (enerf_amd/mc_table.py), as int32 vertex indices; (b - a) x (c - a) points to the side below the threshold.
  * World coordinates: v / (R - 1) * (hi - lo) + lo in fp64, hi - lo in fp32 (extract_geometry's numpy arithmetic).

On CUDA tensors marching_cubes runs the library's kernels (enerf_marching_cubes_*); the vectorised torch statement
`marching_cubes_statement` is the CPU path and the reference the GPU tests hold the kernels to.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import mc_table

MAX_RESOLUTION = 512            # every count and index fits in int32
SLAB_POINTS = 1 << 21           # lattice points per density query on the native route
REF_BLOCK = 128                 # the reference's block edge (extract_fields, S = 128)

_TABLES = {}


def _tables(dev):
    t = _TABLES.get(dev)
    if t is None:
        counts, edges, _max_tri = mc_table.build_tables()
        corner = np.array([mc_table.CORNERS[c] for c in mc_table.EDGE_CORNER], np.int64)
        t = _TABLES[dev] = (torch.from_numpy(counts.astype(np.int64)).to(dev),
                            torch.from_numpy(edges.astype(np.int64)).to(dev),
                            torch.from_numpy(corner).to(dev),
                            torch.tensor(mc_table.EDGE_AXIS, dtype=torch.int64, device=dev))
    return t


def _check_resolution(R):
    R = int(R)
    if R < 2 or R > MAX_RESOLUTION:
        raise ValueError(f"resolution {R}: must be 2 .. {MAX_RESOLUTION}")
    return R


def _check_field(u):
    if u.dim() != 3 or not (u.shape[0] == u.shape[1] == u.shape[2]):
        raise ValueError(f"field of shape {tuple(u.shape)}: [R, R, R] expected")
    if u.dtype != torch.float32:
        raise ValueError(f"field of dtype {u.dtype}: float32 expected")
    return _check_resolution(u.shape[0])


def lattice_step(lo, hi, R):
    """fp32 (hi - lo) / (R - 1) per axis, as torch.linspace computes its step on the CPU."""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return (hi32 - lo32) / np.float32(R - 1)


# ----------------------------------------------------------------------------------------------------------- field
def _field_supported(model, dev):
    from . import fused_network
    if dev.type != "cuda":
        return False
    probe = torch.empty(0, 3, device=dev)
    return fused_network.supported(model, probe, probe)


def _lattice(box, R, x0, nx, pts):
    L.check(L.lib().enerf_mesh_lattice(box, R, x0, nx, pts.data_ptr(), L.stream_handle()), "mesh_lattice")


def lattice_points(lo, hi, R, x0, nx, device):
    """Points of the x-planes [x0, x0 + nx) of the lattice in field order, [nx * R * R, 3] fp32 (the lattice kernel)."""
    R = _check_resolution(R)
    box = (ctypes.c_float * 9)(*[float(v) for v in np.concatenate([np.asarray(lo, np.float32),
                                                                   np.asarray(hi, np.float32), lattice_step(lo, hi, R)])])
    pts = torch.empty(nx * R * R, 3, dtype=torch.float32, device=device)
    _lattice(box, R, x0, nx, pts)
    return pts


def _field_native(model, R, lo, hi, dev):
    from . import fused_network
    from .fused_mlp import pad32
    u = torch.empty(R, R, R, dtype=torch.float32, device=dev)
    nx = min(R, max(1, SLAB_POINTS // (R * R)))
    B = nx * R * R
    box = (ctypes.c_float * 9)(*[float(v) for v in np.concatenate([np.asarray(lo, np.float32),
                                                                   np.asarray(hi, np.float32), lattice_step(lo, hi, R)])])
    pts = torch.empty(B, 3, dtype=torch.float32, device=dev)
    feats = torch.empty(16 * pad32(B) * 2, dtype=torch.float32, device=dev)     # (freed on return: no model scratch)
    flat = u.view(R, R * R)
    for x0 in range(0, R, nx):
        n = min(nx, R - x0)
        _lattice(box, R, x0, n, pts)
        fused_network.density_sigma(model, pts[:n * R * R], out=flat[x0:x0 + n].view(-1), feats=feats)
    return u


def _field_blocks(model, R, lo, hi, dev):
    """The reference's extract_fields: 128^3 blocks of the CPU linspace lattice through model.density."""
    X, Y, Z = (torch.linspace(lo[a], hi[a], R).split(REF_BLOCK) for a in range(3))
    X, Y, Z = list(X), list(Y), list(Z)
    u = torch.empty(R, R, R, dtype=torch.float32, device=dev)
    S = REF_BLOCK
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                val = model.density(pts.to(dev))["sigma"].reshape(len(xs), len(ys), len(zs))
                u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


@torch.no_grad()
def density_field(model, resolution, lo, hi):
    """sigma on the resolution^3 lattice over [lo, hi] (3 floats each) -> u [R, R, R] fp32 on the model's device.
    A model the fused path serves (CUDA, no autocast) takes the lattice kernel and fused_network.density_sigma in slabs
    of at most 2^21 points, at the model's `mlp_precision`; anything else calls model.density in the reference's blocks.
    Nothing is kept after the call (in particular not the model's `_density_scratch`)."""
    R = _check_resolution(resolution)
    lo = [float(np.float32(v)) for v in lo]
    hi = [float(np.float32(v)) for v in hi]
    dev = next(model.parameters()).device
    if _field_supported(model, dev):
        return _field_native(model, R, lo, hi, dev)
    return _field_blocks(model, R, lo, hi, dev)


# ------------------------------------------------------------------------------------------------- marching cubes
def _nonfinite_error(n):
    return ValueError(f"marching_cubes: the field holds {n} non-finite value(s)")


def marching_cubes_statement(u, threshold):
    """The vectorised torch statement of the semantics (any device) -> (vertices [V, 3] fp64, triangles [F, 3] int32)."""
    R = _check_field(u)
    dev = u.device
    thr = float(threshold)
    bad = int((~torch.isfinite(u)).sum())
    if bad:
        raise _nonfinite_error(bad)
    counts, edges, corner, eaxis = _tables(dev)
    above = u.double() > thr
    flags = torch.zeros(R, R, R, 3, dtype=torch.bool, device=dev)
    flags[:-1, :, :, 0] = above[:-1] != above[1:]
    flags[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    flags[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    fl = flags.reshape(-1)
    q = fl.nonzero().squeeze(1)
    p, a = q // 3, q % 3
    stride = torch.tensor([R * R, R, 1], dtype=torch.int64, device=dev)
    uf = u.reshape(-1)
    u0, u1 = uf[p].double(), uf[p + stride[a]].double()
    t = (thr - u0) / (u1 - u0)
    verts = torch.stack([p // (R * R), (p // R) % R, p % R], dim=1).double()
    rows = torch.arange(q.numel(), device=dev)
    verts[rows, a] = verts[rows, a] + t
    vid = torch.cumsum(fl.to(torch.int64), 0) - 1

    ab = above.to(torch.int64)
    n = R - 1
    case = torch.zeros(n, n, n, dtype=torch.int64, device=dev)
    for k, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        case |= ab[dx:dx + n, dy:dy + n, dz:dz + n] << k
    case = case.reshape(-1)
    ntri = counts[case]
    cells = (ntri > 0).nonzero().squeeze(1)
    cc, nt = case[cells], ntri[cells]
    E = edges[cc]                                                       # [cells, MAX_TRI, 3]
    valid = torch.arange(E.shape[1], device=dev)[None, :] < nt[:, None]
    origin = (cells // (n * n)) * R * R + ((cells // n) % n) * R + cells % n
    e = E[valid]                                                        # [F, 3], cell order then table order
    org = origin[:, None].expand(-1, E.shape[1])[valid][:, None]
    off = corner[e]                                                     # [F, 3, 3]
    owner = org + off[..., 0] * R * R + off[..., 1] * R + off[..., 2]
    tris = vid[owner * 3 + eaxis[e]].to(torch.int32)
    return verts, tris.reshape(-1, 3)


def _marching_cubes_native(u, threshold):
    R = _check_field(u)
    u = u.contiguous()
    lib = L.lib()
    nbytes = ctypes.c_uint64(0)
    L.check(lib.enerf_marching_cubes_workspace(R, ctypes.byref(nbytes)), "marching_cubes_workspace")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=u.device)
    totals = torch.empty(3, dtype=torch.int64, device=u.device)
    s = L.stream_handle()
    L.check(lib.enerf_marching_cubes_count(u.data_ptr(), R, float(threshold), ws.data_ptr(), totals.data_ptr(), s),
            "marching_cubes_count")
    V, F, bad = (int(v) for v in totals.tolist())              # the one read-back: both totals and the non-finite count
    if bad:
        raise _nonfinite_error(bad)
    verts = torch.empty(V, 3, dtype=torch.float64, device=u.device)
    tris = torch.empty(F, 3, dtype=torch.int32, device=u.device)
    L.check(lib.enerf_marching_cubes_emit(u.data_ptr(), R, float(threshold), ws.data_ptr(), V, F, verts.data_ptr(),
                                          tris.data_ptr(), s), "marching_cubes_emit")
    return verts, tris


def marching_cubes(u, threshold):
    """u [R, R, R] fp32 -> (vertices [V, 3] fp64 in index space, triangles [F, 3] int32), on u's device.  CUDA tensors
    take the HIP kernels, CPU tensors the torch statement; both give the same arrays.  A non-finite value in u raises
    ValueError."""
    if u.is_cuda:
        return _marching_cubes_native(u, threshold)
    return marching_cubes_statement(u, threshold)


def to_world(vertices, resolution, lo, hi):
    """extract_geometry's mapping: v / (R - 1) * (hi - lo) + lo in fp64, with hi - lo taken in fp32."""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    span = torch.tensor((hi32 - lo32).astype(np.float64), device=vertices.device)
    base = torch.tensor(lo32.astype(np.float64), device=vertices.device)
    return vertices / (resolution - 1.0) * span[None, :] + base[None, :]


def extract_geometry(model, resolution, threshold):
    """-> (vertices [V, 3] fp64 in world coordinates, triangles [F, 3] int32) over model.aabb_infer."""
    box = model.aabb_infer.detach().float().cpu().numpy()
    lo, hi = box[:3], box[3:]
    u = density_field(model, resolution, lo, hi)
    v, f = marching_cubes(u, threshold)
    return to_world(v, int(resolution), lo, hi), f


# ------------------------------------------------------------------------------------------------------------ PLY
def write_ply(path, vertices, triangles):
    """Binary little-endian PLY 1.0: `float x, y, z` (rounded once from fp64) and `list uchar int vertex_indices`."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.asarray(torch.as_tensor(triangles).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    face = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    face["n"] = 3
    face["i"] = f
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(face.tobytes())
    return path


def read_ply(path):
    """Parser of what write_ply writes -> (vertices [V, 3] float32, triangles [F, 3] int32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0", head[:2]
    nv = int(next(line for line in head if line.startswith("element vertex")).split()[2])
    nf = int(next(line for line in head if line.startswith("element face")).split()[2])
    v = np.frombuffer(data, "<f4", nv * 3, end).reshape(nv, 3)
    face = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nf, end + nv * 12)
    assert (face["n"] == 3).all() and end + nv * 12 + nf * 13 == len(data)
    return v, face["i"].reshape(nf, 3)


def harness_save_mesh(harness, save_path, resolution=256, threshold=10):
    """TrainHarness.save_mesh: the query in the harness's regime (as the reference's autocast(enabled=fp16)), the PLY
    written by rank 0 only."""
    import os
    import torch.distributed as dist
    model = harness.model
    if harness.strat_f16 or harness.amp_f16:
        prev = harness._amp_scope()
        try:
            v, f = extract_geometry(model, resolution, threshold)
        finally:
            harness._amp_restore(prev)
    elif harness.fp16:
        with torch.autocast("cuda", dtype=torch.float16):
            v, f = extract_geometry(model, resolution, threshold)
    else:
        v, f = extract_geometry(model, resolution, threshold)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0:
        d = os.path.dirname(save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        write_ply(save_path, v, f)
    return v, f

