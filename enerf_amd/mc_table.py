"""Marching-cubes tables derived from the classification (no table is typed in), and the header csrc/mc_tables.h.

    python -m enerf_amd.mc_table            # rewrite enerf_amd/csrc/mc_tables.h
    python -m enerf_amd.mc_table --check    # exit 1 when the committed header differs from what this derives

Cube of one cell: corner k = (dx, dy, dz) = ((k >> 2) & 1, (k >> 1) & 1, k & 1) (x slowest, like the field), and bit k
of the case index is set when corner k is above the threshold.  Edge e = 4 * axis + j joins corner `EDGE_CORNER[e]` (its
coordinate along `axis` is 0) to that corner + e_axis; the vertex of a crossed edge is owned by that lower corner.

Per case:
  * each of the 6 faces holds 0, 2 or 4 crossed edges.  Two give one segment.  Four (the two above corners on one
    diagonal) give two segments, each cutting off one above corner: the above corners stay apart.  The choice reads the
    face's four corners only, so the two cells that share a face pair its crossings alike and the mesh is watertight;
  * every crossed edge lies on two faces, so the segments chain into closed loops (asserted);
  * each loop is fan-triangulated from its lowest-numbered edge;
  * each segment is directed along n x N_f (n: in the face, from the above side to the below side; N_f: the face's
    outward normal), which makes every triangle's (b - a) x (c - a) point to the side below the threshold.
"""
import os
import sys

import numpy as np

CORNERS = [((k >> 2) & 1, (k >> 1) & 1, k & 1) for k in range(8)]


def _corner(c):
    return (c[0] << 2) | (c[1] << 1) | c[2]


def _edges():
    """[(lower corner, axis)] for e = 4 * axis + j, j running over the other two coordinates (the slower one first)."""
    out = []
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        for j in range(4):
            c = [0, 0, 0]
            c[others[0]], c[others[1]] = (j >> 1) & 1, j & 1
            out.append((_corner(c), axis))
    return out


EDGES = _edges()
EDGE_CORNER = [c for c, _ in EDGES]
EDGE_AXIS = [a for _, a in EDGES]


def _edge_ends(e):
    c, a = EDGES[e]
    return c, c | (1 << (2 - a))


def _midpoint(e):
    c0, c1 = _edge_ends(e)
    return (np.array(CORNERS[c0], float) + np.array(CORNERS[c1], float)) / 2


def _faces():
    """[(axis, side, [4 corners], [4 edges])]."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [k for k in range(8) if CORNERS[k][axis] == side]
            es = [e for e in range(12) if EDGE_AXIS[e] != axis and CORNERS[EDGE_CORNER[e]][axis] == side]
            out.append((axis, side, cs, es))
    return out


FACES = _faces()


def crossed_edges(case):
    above = [(case >> k) & 1 for k in range(8)]
    return [e for e in range(12) if above[_edge_ends(e)[0]] != above[_edge_ends(e)[1]]]


def _face_segments(case, face):
    """Directed segments (e_from, e_to) of one face."""
    axis, side, cs, es = face
    above = {k: (case >> k) & 1 for k in cs}
    crossed = [e for e in es if above[_edge_ends(e)[0]] != above[_edge_ends(e)[1]]]
    assert len(crossed) in (0, 2, 4), (case, face, crossed)
    if not crossed:
        return []
    pairs = []                                   # (edge a, edge b, n: from the above side to the below side)
    if len(crossed) == 2:
        a_c = np.mean([CORNERS[k] for k in cs if above[k]], axis=0)
        b_c = np.mean([CORNERS[k] for k in cs if not above[k]], axis=0)
        pairs.append((crossed[0], crossed[1], b_c - a_c))
    else:
        for k in cs:
            if above[k]:                         # cut off this above corner: its two face edges
                ek = [e for e in es if k in _edge_ends(e)]
                m = (_midpoint(ek[0]) + _midpoint(ek[1])) / 2
                pairs.append((ek[0], ek[1], m - np.array(CORNERS[k], float)))
    n_face = np.zeros(3)
    n_face[axis] = 1.0 if side == 1 else -1.0
    out = []
    for a, b, n in pairs:
        n = n.copy()
        n[axis] = 0.0
        t = np.cross(n, n_face)
        d = _midpoint(b) - _midpoint(a)
        assert abs(float(np.dot(d, t))) > 1e-9
        out.append((a, b) if np.dot(d, t) > 0 else (b, a))
    return out


def case_loops(case):
    """Closed loops of crossed edges of one case, each starting at its lowest edge, loops by their first edge."""
    nxt = {}
    for f in FACES:
        for a, b in _face_segments(case, f):
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == crossed_edges(case) and sorted(nxt.values()) == crossed_edges(case), case
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, f"case {case}: loop from edge {start} does not close"
        assert len(loop) >= 3, (case, loop)
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_tables():
    """-> (counts [256] uint8, edges [256, MAX_TRI, 3] int8 padded with -1, MAX_TRI)."""
    tri = [case_triangles(c) for c in range(256)]
    max_tri = max(len(t) for t in tri)
    counts = np.array([len(t) for t in tri], np.uint8)
    edges = np.full((256, max_tri, 3), -1, np.int8)
    for c, t in enumerate(tri):
        if t:
            edges[c, :len(t)] = np.array(t, np.int8)
    return counts, edges, max_tri


def header_text():
    counts, edges, max_tri = build_tables()
    lines = [
        "// mc_tables.h -- GENERATED by enerf_amd/mc_table.py (python -m enerf_amd.mc_table); do not edit.",
        "// Corner k = ((k >> 2) & 1, (k >> 1) & 1, k & 1) (x slowest); bit k of a case is set when corner k is above the",
        "// threshold.  Edge e joins corner kMcEdgeCorner[e] to that corner + e_{kMcEdgeAxis[e]}.  Triangles: edge ids, wound so",
        "// that (b - a) x (c - a) points to the side below the threshold.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#ifndef ENERF_MC_CONST",
        "#define ENERF_MC_CONST static const",
        "#endif",
        "",
        f"#define ENERF_MC_MAX_TRI {max_tri}",
        "",
        "ENERF_MC_CONST uint8_t kMcEdgeCorner[12] = {" + ", ".join(str(c) for c in EDGE_CORNER) + "};",
        "ENERF_MC_CONST uint8_t kMcEdgeAxis[12] = {" + ", ".join(str(a) for a in EDGE_AXIS) + "};",
        "ENERF_MC_CONST uint8_t kMcTriCount[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(v)) for v in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append(f"ENERF_MC_CONST int8_t kMcTriEdges[256][{max_tri * 3}] = {{")
    for c in range(256):
        lines.append("    {" + ", ".join(str(int(v)) for v in edges[c].reshape(-1)) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_tables.h")


def main(argv):
    text = header_text()
    print(f"[mc_table] largest triangle count of a case: {build_tables()[2]}")
    if "--check" in argv:
        with open(HEADER) as f:
            same = f.read() == text
        print(f"[mc_table] {HEADER}: {'up to date' if same else 'DIFFERS'}")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"[mc_table] wrote {HEADER}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
