"""Mint tests/golden/ref_mesh_field.npz from the reference's own mesh-export Python (this container only).

    cd <repo> && python -B tests/refcheck/mint_mesh_golden.py

TEST INFRASTRUCTURE ONLY.  Runs the reference's `extract_fields` (nerf/utils.py:219-234) on a seeded cuda_ray = False
NeRFNetwork at R = 130 (its 128^3 blocks split 128 + 2 on every axis) with `model.density` as the query, on the CPU with the
C oracle behind the grid encoder (oracle/ref_import.py), and `extract_geometry` (:237-249) with `mcubes` stubbed: the
stub returns fixed index-space vertices, so what is recorded is the reference's world mapping of them.  Stored: the seed
recipe (the model is rebuilt from it, not stored), the field's SHA-256 and the planes next to the block boundary, the
stub's vertices and the reference's world vertices.
"""
import hashlib
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE,STRICT"          # the CPU settings tests/conftest.py pins for the suite
os.environ["OMP_NUM_THREADS"] = "8"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from oracle.make_golden import det_fill_  # noqa: E402

R, BOUND, SEED, LO, HI, THRESHOLD = 130, 1, 71, -0.5, 0.5, 10
PLANES = (127, 128)


def main():
    ref_import.install()
    from nerf.network import NeRFNetwork
    from nerf import utils
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", bound=BOUND, cuda_ray=False, out_dim_color=3)
    det_fill_(list(model.parameters()), SEED, LO, HI)
    model.eval()
    aabb = model.aabb_infer

    def query(pts):
        return model.density(pts)["sigma"]

    u = utils.extract_fields(aabb[:3], aabb[3:], R, query)
    assert u.shape == (R, R, R) and u.dtype == np.float32

    # extract_geometry with mcubes stubbed: capture u, hand back fixed index-space vertices
    g = np.random.default_rng(SEED)
    stub_v = np.concatenate([g.uniform(0, R - 1, (64, 3)), np.array([[0, 0, 0], [R - 1, R - 1, R - 1], [0.5, 64.25, 129]])])
    stub_f = np.zeros((1, 3), np.int64)
    seen = {}

    def marching_cubes(field, threshold):
        seen["u"], seen["thr"] = field, threshold
        return stub_v.copy(), stub_f

    sys.modules["mcubes"].marching_cubes = marching_cubes
    world, tris = utils.extract_geometry(aabb[:3], aabb[3:], R, THRESHOLD, query)
    assert np.array_equal(seen["u"].view(np.uint32), u.view(np.uint32)) and seen["thr"] == THRESHOLD
    out = os.path.join(ROOT, "tests", "golden", "ref_mesh_field.npz")
    np.savez_compressed(out, resolution=R, bound=BOUND, seed=SEED, fill_lo=LO, fill_hi=HI, aabb=aabb.numpy(),
                        sha256=np.frombuffer(hashlib.sha256(u.tobytes()).digest(), np.uint8), planes=np.array(PLANES),
                        u_x=u[list(PLANES)], u_y=u[:, list(PLANES)], u_z=u[:, :, list(PLANES)],
                        stub_vertices=stub_v, world_vertices=world)
    print(f"wrote {out}: u in [{u.min():.4g}, {u.max():.4g}], median {np.median(u):.4g}")


if __name__ == "__main__":
    main()
