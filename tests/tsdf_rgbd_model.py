"""numpy float32 model of gaustudio_amd.tsdf_rgbd.ColorTSDFVolume (csrc/gsr_tsdf_rgbd.hip).  TEST INFRASTRUCTURE ONLY.

The model is the authority for the semantics: it states every operation in the order the kernels perform it, in float32 with
one rounding per operation (the library is built with -ffp-contract=off and correctly rounded divide / sqrt), so device
results are compared with it by np.array_equal.  It restates Open3D's published algorithm for ScalableTSDFVolume::Integrate,
UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier and ::ExtractTriangleMesh (Open3D itself is not installed
here: parity with the library is unpinned, tests/test_tsdf_rgbd_open3d.py runs where it is), with this project's choices:

  * voxel (i, j, k), any sign, has its centre at ((i, j, k) + 0.5) * voxel_length; blocks are 8^3 voxels (Open3D: 16^3 --
    the block edge only changes which far-from-surface voxels hold tsdf = 1);
  * a voxel holds tsdf (in units of sdf_trunc), weight and colour (0..255), all float32, zero until observed;
  * marching cubes with the project's derived tables (gaustudio_amd/csrc/gen_mc_tables.py), one shared vertex per crossed edge,
    blocks emitted in key order, voxels of a block with x fastest.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaustudio_amd", "csrc"))
import gen_mc_tables as _tables  # noqa: E402

F = np.float32
OWNER = [0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3]      # per cube edge: the corner that owns it (the edge's minimum corner)
AXIS = [0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2]       # and its axis
BLOCK_LIMIT = 1048575                             # block coordinates of the 21-bit key fields


def intrinsic4(intrinsic):
    k = np.asarray(intrinsic, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    return k.astype(F)


def clean_depth(depth, depth_trunc):
    """mesh.py:556-560: non-finite, negative and > depth_trunc -> 0 (no observation)."""
    d = np.asarray(depth, dtype=F)
    with np.errstate(invalid="ignore"):
        ok = (d > F(0)) & (d <= F(depth_trunc)) & (d <= F(3.4028235e38))
    return np.where(ok, d, F(0)).astype(F)


def quantise_color(color):
    """uint8 [H,W,3] as it is; float [H,W,3] or [3,H,W] in [0,1] by uint8(clip(x * 255, 0, 255)), truncating (mesh.py:532-534;
    NaN -> 0).  Returns float32 [H,W,3] holding the integers 0..255."""
    c = np.asarray(color)
    if c.dtype == np.uint8:
        return c.astype(F)
    c = c.astype(F)
    if c.ndim == 3 and c.shape[0] == 3 and c.shape[2] != 3:
        c = np.transpose(c, (1, 2, 0))
    with np.errstate(invalid="ignore"):
        q = np.fmin(np.fmax(c * F(255.0), F(0)), F(255.0))
    return q.astype(np.int32).astype(F)


def _xform(M, r, x, y, z):
    return ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]


class ModelVolume:
    def __init__(self, voxel_length=0.02, sdf_trunc=0.04, depth_sampling_stride=4):
        self.vl, self.tr, self.stride = F(voxel_length), F(sdf_trunc), int(depth_sampling_stride)
        self.blocks = {}                # (bx, by, bz) -> [tsdf [512], weight [512], color [512, 3]] float32, x fastest

    # ------------------------------------------------------------------ touch
    def touched_blocks(self, depth, intrinsic, extrinsic, depth_trunc):
        """The set of blocks a frame opens: for every pixel (u, v) on the stride grid with cleaned depth d > 0 the blocks that
        intersect the box [p - sdf_trunc, p + sdf_trunc], p = E^-1 ((u - cx) d / fx, (v - cy) d / fy, d).  E^-1 is computed in
        float64 and used as float32."""
        K = intrinsic4(intrinsic)
        fx, fy, cx, cy = K
        Einv = np.linalg.inv(np.asarray(extrinsic, dtype=np.float64))[:3].astype(F)
        d = clean_depth(depth, depth_trunc)[::self.stride, ::self.stride]
        v, u = np.meshgrid(np.arange(d.shape[0]) * self.stride, np.arange(d.shape[1]) * self.stride, indexing="ij")
        m = d > 0
        d, u, v = d[m], u[m].astype(F), v[m].astype(F)
        x = ((u - cx) * d) / fx
        y = ((v - cy) * d) / fy
        bs = F(8.0) * self.vl
        lo, hi, ok = [], [], np.ones(d.shape, bool)
        for a in range(3):
            p = _xform(Einv, a, x, y, d)
            fl, fh = np.floor((p - self.tr) / bs), np.floor((p + self.tr) / bs)
            ok &= (fl >= -BLOCK_LIMIT) & (fl <= BLOCK_LIMIT) & (fh >= -BLOCK_LIMIT) & (fh <= BLOCK_LIMIT)
            lo.append(fl)
            hi.append(fh)
        boxes = np.stack(lo + hi, axis=1)[ok].astype(np.int64)
        out = set()
        for b in np.unique(boxes, axis=0):
            for bz in range(b[2], b[5] + 1):
                for by in range(b[1], b[4] + 1):
                    for bx in range(b[0], b[3] + 1):
                        out.add((bx, by, bz))
        return out

    # ------------------------------------------------------------------ integrate
    def integrate(self, depth, color, intrinsic, extrinsic, depth_trunc=5.0):
        """One frame.  Returns the set of blocks it touched (every voxel of these, and no other, is offered the frame)."""
        touched = sorted(self.touched_blocks(depth, intrinsic, extrinsic, depth_trunc))
        for b in touched:
            if b not in self.blocks:
                self.blocks[b] = [np.zeros(512, F), np.zeros(512, F), np.zeros((512, 3), F)]
        if not touched:
            return set()
        K = intrinsic4(intrinsic)
        fx, fy, cx, cy = K
        E = np.asarray(extrinsic, dtype=np.float64)[:3].astype(F)
        dimg = clean_depth(depth, depth_trunc)
        cimg = quantise_color(color)
        H, W = dimg.shape
        assert cimg.shape == (H, W, 3)
        local = np.arange(512)
        l3 = np.stack([local & 7, (local >> 3) & 7, local >> 6], axis=1)
        ijk = np.asarray(touched, dtype=np.int64)[:, None, :] * 8 + l3[None]           # [n, 512, 3]
        X, Y, Z = [(ijk[..., a].astype(F) + F(0.5)) * self.vl for a in range(3)]
        cz = _xform(E, 2, X, Y, Z)
        ok = cz > 0                                                                    # behind the camera: skipped
        czs = np.where(ok, cz, F(1))
        uf = ((_xform(E, 0, X, Y, Z) * fx) / czs + cx) + F(0.5)
        vf = ((_xform(E, 1, X, Y, Z) * fy) / czs + cy) + F(0.5)
        with np.errstate(invalid="ignore"):
            ok &= (uf >= F(0.0001)) & (uf < F(W) - F(0.0001)) & (vf >= F(0.0001)) & (vf < F(H) - F(0.0001))
        u = np.where(ok, uf, F(0)).astype(np.int32)
        v = np.where(ok, vf, F(0)).astype(np.int32)
        d = dimg[v, u]
        ok &= d > 0
        a, b = (u.astype(F) - cx) / fx, (v.astype(F) - cy) / fy
        mult = np.sqrt((a * a + b * b) + F(1))
        sdf = (d - cz) * mult
        ok &= sdf > -self.tr
        t = np.minimum(F(1), sdf / self.tr)
        rgb = cimg[v, u]
        assert t.dtype == F and mult.dtype == F and uf.dtype == F
        for n, blk in enumerate(touched):
            tsdf, w, col = self.blocks[blk]
            m = ok[n]
            w1 = w[m] + F(1)
            tsdf[m] = (tsdf[m] * w[m] + t[n][m]) / w1
            col[m] = (col[m] * w[m][:, None] + rgb[n][m]) / w1[:, None]
            w[m] = w1
        return set(touched)

    # ------------------------------------------------------------------ inspection
    def export_voxels(self):
        """(coords [m,3] int32, tsdf [m], weight [m], color [m,3]) of the voxels with weight > 0, sorted by (z, y, x)."""
        local = np.arange(512)
        l3 = np.stack([local & 7, (local >> 3) & 7, local >> 6], axis=1)
        cs, ts, ws, cols = [np.zeros((0, 3), np.int64)], [np.zeros(0, F)], [np.zeros(0, F)], [np.zeros((0, 3), F)]
        for b, (tsdf, w, col) in self.blocks.items():
            m = w > 0
            cs.append((np.asarray(b, dtype=np.int64)[None] * 8 + l3)[m])
            ts.append(tsdf[m]); ws.append(w[m]); cols.append(col[m])
        c, t, w, col = np.concatenate(cs), np.concatenate(ts), np.concatenate(ws), np.concatenate(cols)
        order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
        return c[order].astype(np.int32), t[order], w[order], col[order]

    def voxel(self, i, j, k):
        """(tsdf, weight, color [3]) of one voxel (zeros when its block was never opened)."""
        b = self.blocks.get((i >> 3, j >> 3, k >> 3))
        if b is None:
            return F(0), F(0), np.zeros(3, F)
        l = ((k & 7) << 6) | ((j & 7) << 3) | (i & 7)
        return b[0][l], b[1][l], b[2][l].copy()

    # ------------------------------------------------------------------ mesh
    def extract_triangle_mesh(self, min_weight=0.0):
        """(vertices [nv,3] f32, triangles [nt,3] i32, colors [nv,3] f32 in [0,1]).  A cube with corner voxels
        (i..i+1, j..j+1, k..k+1) is meshed iff all 8 have weight > 0 and weight >= min_weight; a corner is inside iff
        tsdf < 0; a vertex lies at r = |f0| / (|f0| + |f1|) along its edge from the owning voxel's centre and carries
        clamp(c0 + r (c1 - c0), min(c0, c1), max(c0, c1)) / 255."""
        empty = (np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros((0, 3), F))
        if not self.blocks:
            return empty
        table, edge_mask = _tables.build()
        bl = np.asarray(sorted(self.blocks), dtype=np.int64)           # key order = lexicographic (bx, by, bz)
        org = bl.min(0) * 8
        dim = (bl.max(0) - bl.min(0) + 1) * 8 + 1                      # one layer of never-observed voxels on the far side
        tsdf, wgt, col = np.zeros(dim, F), np.zeros(dim, F), np.zeros((*dim, 3), F)
        rank = np.full(dim, -1, np.int64)                              # emission rank of a voxel: block rank * 512 + local
        local = np.arange(512)
        lx, ly, lz = local & 7, (local >> 3) & 7, local >> 6
        for r, b in enumerate(map(tuple, bl)):
            o = np.asarray(b) * 8 - org
            t, w, c = self.blocks[b]
            tsdf[o[0] + lx, o[1] + ly, o[2] + lz] = t
            wgt[o[0] + lx, o[1] + ly, o[2] + lz] = w
            col[o[0] + lx, o[1] + ly, o[2] + lz] = c
            rank[o[0] + lx, o[1] + ly, o[2] + lz] = r * 512 + local
        usable = (wgt > 0) & (wgt >= F(min_weight))
        inside = tsdf < 0
        n = dim - 1
        ok = np.ones(n, bool)
        case = np.zeros(n, np.int64)
        for i, (dx, dy, dz) in enumerate(_tables.CORNERS):
            sl = (slice(dx, dx + n[0]), slice(dy, dy + n[1]), slice(dz, dz + n[2]))
            ok &= usable[sl]
            case |= inside[sl].astype(np.int64) << i
        case[~ok | (case == 255)] = 0
        flags = np.zeros(dim, np.int64)
        em = np.asarray(edge_mask)[case]
        for e in range(12):
            dx, dy, dz = _tables.CORNERS[OWNER[e]]
            flags[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]] |= ((em >> e) & 1) << AXIS[e]
        # vertices: owning voxels in emission order, axes 0, 1, 2 inside a voxel
        own = np.argwhere(flags != 0)
        own = own[np.argsort(rank[tuple(own.T)], kind="stable")]
        assert (rank[tuple(own.T)] >= 0).all()
        vbase = np.full(dim, -1, np.int64)
        verts, cols = [], []
        half = F(0.5)
        for o in own:
            o = tuple(o)
            fl = flags[o]
            vbase[o] = len(verts)
            base = [(F(o[a] + org[a]) + half) * self.vl for a in range(3)]
            f0, c0 = tsdf[o], col[o]
            for a in range(3):
                if not (fl >> a) & 1:
                    continue
                q = list(o)
                q[a] += 1
                q = tuple(q)
                a0, a1 = np.abs(f0), np.abs(tsdf[q])
                p = list(base)
                p[a] = p[a] + (a0 * self.vl) / (a0 + a1)
                r = a0 / (a0 + a1)
                c1 = col[q]
                c = np.minimum(np.maximum(c0 + r * (c1 - c0), np.minimum(c0, c1)), np.maximum(c0, c1))
                verts.append(p)
                cols.append(c / F(255.0))
        # triangles: anchor voxels in emission order, table order inside a cube
        anchors = np.argwhere(case != 0)
        anchors = anchors[np.argsort(rank[tuple(anchors.T)], kind="stable")]
        tris = []
        for v in anchors:
            for tri in table[case[tuple(v)]]:
                idx = []
                for e in tri:
                    oc = tuple(v + np.asarray(_tables.CORNERS[OWNER[e]]))
                    idx.append(vbase[oc] + bin(int(flags[oc]) & ((1 << AXIS[e]) - 1)).count("1"))
                tris.append(idx)
        if not tris:
            return empty
        out_v = np.asarray(verts, dtype=F).reshape(-1, 3)
        out_c = np.asarray(cols, dtype=F).reshape(-1, 3)
        assert out_v.dtype == F and out_c.dtype == F
        return out_v, np.asarray(tris, dtype=np.int32).reshape(-1, 3), out_c


def vertex_normals(vertices, faces):
    """Unnormalised area-weighted sum of face normals per vertex, normalised -- for plausibility checks only (the device's
    fixed-order float32 sum is compared against mesh_raster, not against this)."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, f[:, c], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
