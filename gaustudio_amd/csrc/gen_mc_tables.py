#!/usr/bin/env python
"""Generates gsr_mc_tables.h: the 256-case marching-cubes triangle table and the cube geometry (corner offsets, the owner and
the axis of every edge) that every marching-cubes extractor of the library reads: the block kernels of the two sparse
volumes (csrc/gsr_block_volume.h, csrc/gsr_tsdf.hip) and the dense-grid kernels of csrc/gsr_psr.hip.  Under hipcc the tables
are statically initialised __constant__ arrays: compile-time data of the code object, nothing to upload at run time.

The tables are DERIVED here, not transcribed: for every sign configuration of the eight cube corners the
isosurface inside the cube is assembled from oriented segments on the six faces and the resulting closed loops are
fan-triangulated from an apex chosen so that no fan diagonal lies in a cube face (see case_triangles).  Corner / edge numbering is the usual one (Lorensen & Cline 1987 as popularised by P. Bourke):

    corners  0:(0,0,0) 1:(1,0,0) 2:(1,1,0) 3:(0,1,0) 4:(0,0,1) 5:(1,0,1) 6:(1,1,1) 7:(0,1,1)
    edges    0:0-1 1:1-2 2:2-3 3:3-0 4:4-5 5:5-6 6:6-7 7:7-4 8:0-4 9:1-5 10:2-6 11:3-7

bit i of the case index is set when corner i is INSIDE (tsdf < 0).  Faces are walked counter-clockwise seen from
outside the cube; on a face a segment runs from the crossing where the boundary walk ENTERS a run of inside corners to
the crossing where it leaves it, which makes every loop wind counter-clockwise seen from the outside (tsdf > 0) side:
triangle normals point from inside to outside (checked numerically for all 256 cases, tests/test_tsdf.py).  On an ambiguous face (inside corners on a diagonal) the two inside
corners are cut off separately; the rule only looks at the face's four signs, so both cubes sharing the face agree and
the mesh is watertight.  A triangle edge that is not one of these face segments is a diagonal of a loop; it never joins two
cube edges of one cube face, so it runs through the cube's interior and belongs to this cube alone: every edge of the mesh
is used once per direction, on ambiguous faces too.  tests/test_tsdf.py checks orientation and the diagonals for all 256
cases, and closedness on smooth and on random sign fields.
"""
import os

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
EDGE_OF = {}
for _i, (_a, _b) in enumerate(EDGES):
    EDGE_OF[(_a, _b)] = _i
    EDGE_OF[(_b, _a)] = _i
# faces as corner cycles, counter-clockwise when seen from OUTSIDE the cube
FACES = [(0, 3, 2, 1),   # z = 0, outward normal -z
         (4, 5, 6, 7),   # z = 1, +z
         (0, 1, 5, 4),   # y = 0, -y
         (2, 3, 7, 6),   # y = 1, +y
         (0, 4, 7, 3),   # x = 0, -x
         (1, 2, 6, 5)]   # x = 1, +x


def face_segments(case, face):
    """Directed segments (edge_from, edge_to) on one face: for every maximal run of inside corners met while walking
    the face boundary counter-clockwise (seen from outside), from the crossing that enters the run to the one
    that leaves it."""
    inside = [(case >> c) & 1 for c in face]
    segs = []
    for i in range(4):
        # maximal run of inside corners starting at i (previous corner outside)
        if inside[i] and not inside[(i - 1) % 4]:
            j = i
            while inside[(j + 1) % 4] and (j + 1 - i) < 3:
                j += 1
            enter = EDGE_OF[(face[(i - 1) % 4], face[i % 4])]          # crossing where the walk enters the run
            leave = EDGE_OF[(face[j % 4], face[(j + 1) % 4])]          # crossing where it leaves it
            segs.append((enter, leave))
    return segs


def share_face(e0, e1):
    """True when cube edges e0 and e1 lie on a common cube face."""
    cs = [CORNERS[c] for c in EDGES[e0] + EDGES[e1]]
    return any(len({c[d] for c in cs}) == 1 for d in range(3))


def case_triangles(case):
    """Triangles of one case as triples of cube edges.  Every loop is a fan from one of its vertices.  A fan diagonal that
    joined two cube edges of one cube face would lie IN that face; on an ambiguous face the neighbouring cube's loop can
    carry the same diagonal, and the two cubes would then emit coplanar triangles that share it in the same direction (a
    directed edge used twice, four triangles on one edge).  The apex is therefore the first loop vertex whose diagonals
    all join cube edges without a common face; every loop of the 256 cases has one."""
    if case in (0, 255):
        return []
    nxt = {}
    for f in FACES:
        for a, b in face_segments(case, f):
            assert a not in nxt, (case, a)
            nxt[a] = b
    tris = []
    seen = set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        seen.add(start)
        e = nxt[start]
        while e != start:
            loop.append(e)
            seen.add(e)
            e = nxt[e]
        assert 3 <= len(loop) <= 12, (case, loop)
        n = len(loop)
        apex = next(s for s in range(n) if not any(share_face(loop[s], loop[(s + k) % n]) for k in range(2, n - 1)))
        loop = loop[apex:] + loop[:apex]              # a rotation: the orientation stays
        for k in range(1, n - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))
    return tris


def build():
    table = [case_triangles(c) for c in range(256)]
    edge_mask = [0] * 256
    for c, tris in enumerate(table):
        for t in tris:
            for e in t:
                edge_mask[c] |= 1 << e
    return table, edge_mask


def edge_geometry():
    """Per cube edge the corner that owns it and its axis.  A vertex on an edge is stored once, with the voxel (or grid node) at
    the edge's end with the smaller coordinates: the owner; the axis is the coordinate in which the two ends differ."""
    owner, axis = [], []
    for a, b in EDGES:
        diff = [d for d in range(3) if CORNERS[a][d] != CORNERS[b][d]]
        assert len(diff) == 1, (a, b)
        owner.append(min(a, b, key=lambda c: CORNERS[c]))
        axis.append(diff[0])
    # the values the kernels were written against
    assert owner == [0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3], owner
    assert axis == [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2], axis
    return owner, axis


def header_text():
    table, edge_mask = build()
    owner, axis = edge_geometry()
    maxt = max(len(t) for t in table)
    out = ["// gsr_mc_tables.h -- GENERATED by gen_mc_tables.py (derived marching-cubes tables; do not edit).",
           "#pragma once",
           "#include <stdint.h>",
           f"#define GSR_MC_MAX_TRIS {maxt}",
           "// device code reads the tables from constant memory of its own code object; they are never written",
           "#ifdef __HIPCC__",
           "#define GSR_MC_TABLE static __device__ __constant__ const",
           "#else",
           "#define GSR_MC_TABLE static const",
           "#endif",
           "// cube corner offsets and, per cube edge, the corner that owns it (the end with the smaller coordinates) and its axis",
           "GSR_MC_TABLE int gsr_mc_corner[8][3] = {" + ", ".join("{%d, %d, %d}" % c for c in CORNERS) + "};",
           "GSR_MC_TABLE uint8_t gsr_mc_edge_owner[12] = {" + ", ".join(str(v) for v in owner) + "};",
           "GSR_MC_TABLE uint8_t gsr_mc_edge_axis[12] = {" + ", ".join(str(v) for v in axis) + "};",
           "// number of triangles per case",
           "GSR_MC_TABLE uint8_t gsr_mc_ntris[256] = {" + ", ".join(str(len(t)) for t in table) + "};",
           "// bit e set: edge e carries a vertex in this case",
           "GSR_MC_TABLE uint16_t gsr_mc_edge_mask[256] = {" + ", ".join(str(m) for m in edge_mask) + "};",
           "// triangles as edge triples, padded with 255",
           f"GSR_MC_TABLE uint8_t gsr_mc_tris[256][{3 * maxt}] = {{"]
    for t in table:
        flat = [e for tri in t for e in tri]
        flat += [255] * (3 * maxt - len(flat))
        out.append("\t{" + ", ".join(str(v) for v in flat) + "},")
    out.append("};")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gsr_mc_tables.h")
    with open(path, "w") as f:
        f.write(header_text())
    t, _ = build()
    print("wrote", path, "max triangles per case:", max(len(x) for x in t), "total:", sum(len(x) for x in t))
