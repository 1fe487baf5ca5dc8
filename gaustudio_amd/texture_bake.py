"""Vertex-colour baking on the GPU (csrc/gsr_mesh_bake.hip): what gaustudio/scripts/texture_mesh.py (`gs-texture-mesh`) does
to colour a mesh from posed photographs -- per view: rasterize, keep the visible faces that face the camera, project their
vertices, look the colours up with grid_sample; a later view overwrites an earlier one.

    baker = TextureBaker(vertices, faces, sampling="reference")        # wraps a MeshRasterizer; ROCm tensors only
    st = baker.add_view(image, intrinsics, extrinsics, strict=True)    # rasterize -> visible_faces -> select -> sample
    colors, baked_by = baker.vertex_colors, baker.baked_by             # [V,3] f32 (0 where never baked), [V] int32 (-1)
    colors, baked_by, stats = bake_vertex_colors(vertices, faces, views)     # views: (image, intrinsics, extrinsics), in order

Contract and the reference's quirks (the flipped screen camera, the W - 1 normalisation under align_corners=False that puts
its lookup about one pixel off, vertices behind the camera): INTEGRATION.md s21.  sampling="exact" looks up at the vertex's
own pixel instead.  The result feeds formats.write_ply_mesh(vertex_colors=...), voxelize.voxel_seeds(colors="closest") and
mesh_init.mesh_seeds.  Forward only, deterministic, no CPU fallback; every call runs on the current stream of the mesh's device.
"""
import torch

from ._abi import call, on_rocm, same_device
from .mesh_raster import MeshRasterizer, _host_f32
from .voxelize import _mesh

SAMPLING = ("reference", "exact")
COS_LIMIT = -0.05                   # texture_mesh.py:121


_ERRORS = {-2: "{what}: invalid argument (a bad size, a matrix that is not finite or singular intrinsics)"}


class BakeStats:
    """What one view did: visible_faces (faces that own a pixel), selected_faces (of those, cos < -0.05), baked_vertices
    (vertices this view coloured) and mean_cos (the mean of cos over the visible faces, the script's orientation check; NaN
    when no face is visible).  The four values are computed on the device; the first attribute read fetches them (one
    read-back), which add_view(strict=True) has already done."""

    def __init__(self, raw):
        self._raw, self._host = raw, None

    def _get(self, i):
        if self._host is None:
            self._host = self._raw.cpu().numpy()
        return self._host[i]

    visible_faces = property(lambda self: int(self._get(0)))
    selected_faces = property(lambda self: int(self._get(1)))
    baked_vertices = property(lambda self: int(self._get(2)))
    mean_cos = property(lambda self: float(self._get(3)))

    def __repr__(self):
        return (f"BakeStats(visible_faces={self.visible_faces}, selected_faces={self.selected_faces}, "
                f"baked_vertices={self.baked_vertices}, mean_cos={self.mean_cos:.6g})")


def _image(image, dev):
    """float32 [H,W,3] on `dev`; uint8 is converted (x / 255)."""
    if not torch.is_tensor(image):
        raise TypeError("image must be a torch tensor")
    if image.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"image must be float32 or uint8, got {image.dtype}")
    if image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"image must have shape [H, W, 3], got {list(image.shape)}")
    on_rocm(ValueError, image=image)
    same_device(dev, image=image)
    if image.dtype == torch.uint8:
        image = image.to(torch.float32) / 255.0
    return image.detach().contiguous()


class TextureBaker:
    """Bakes per-vertex colours into one device mesh, a view at a time.  vertices [V,3] float32, faces [F,3] int32 / int64,
    on a ROCm device."""

    def __init__(self, vertices, faces, sampling="reference"):
        if sampling not in SAMPLING:
            raise ValueError(f"sampling must be 'reference' or 'exact', got {sampling!r}")
        dev = _mesh(vertices, faces, vertex_dtypes=(torch.float32,))
        self.sampling = sampling
        self.raster = MeshRasterizer(vertices.detach(), faces.detach())
        self.device = dev
        V = self.raster.num_verts
        self.vertex_colors = torch.zeros((V, 3), dtype=torch.float32, device=dev)
        self.baked_by = torch.full((V,), -1, dtype=torch.int32, device=dev)
        self._stamp = torch.full((V,), -1, dtype=torch.int32, device=dev)      # set once per bake: no per-view clear
        self.num_views = 0
        self.last_cos = None

    # the two kernels, callable on their own (tests, tools/texture_bake_timing.py)
    def select(self, visible, extrinsics, seq, return_cos=True):
        """gsr_mesh_bake_select for the faces with visible[f] (bool / uint8 [F]): stamps the vertices of the selected faces
        with `seq`; returns cos [F] float32 (NaN where not visible), or None."""
        r = self.raster
        if not torch.is_tensor(visible) or visible.dtype not in (torch.bool, torch.uint8) or tuple(visible.shape) != (r.num_faces,):
            raise TypeError(f"visible must be a bool or uint8 tensor of shape [{r.num_faces}]")
        same_device(self.device, visible=visible)
        E = _host_f32("extrinsics", extrinsics, (4, 4))
        vis = visible.to(torch.uint8).contiguous()
        cos = torch.empty(r.num_faces, dtype=torch.float32, device=self.device) if return_cos else None
        call("gsr_mesh_bake_select", self.device, r.verts, r.num_verts, r.faces, r.num_faces, vis, E, int(seq), self._stamp, cos,
             errors=_ERRORS)
        return cos

    def sample(self, image, intrinsics, extrinsics, seq):
        """gsr_mesh_bake_sample for the vertices stamped `seq`: writes vertex_colors and baked_by."""
        img = _image(image, self.device)
        K = _host_f32("intrinsics", intrinsics, (3, 3))
        E = _host_f32("extrinsics", extrinsics, (4, 4))
        r = self.raster
        call("gsr_mesh_bake_sample", self.device, r.verts, r.num_verts, self._stamp, int(seq), K, E, img, img.shape[0], img.shape[1],
             self.sampling == "exact", self.vertex_colors, self.baked_by, errors=_ERRORS)

    def add_view(self, image, intrinsics, extrinsics, strict=True):
        """One iteration of texture_mesh.py:76-141.  image [H,W,3] float32 in [0,1] (or uint8), intrinsics [3,3], extrinsics
        [4,4] world-to-camera in OpenCV axes; the mesh is rasterized at the image's size.  Returns BakeStats.  strict=True
        raises ValueError when mean_cos >= 0 (the script's assert at :120: the mesh is inside out, or the pose is not
        world-to-camera), before anything is baked; it costs one read-back, strict=False skips it."""
        img = _image(image, self.device)
        H, W = int(img.shape[0]), int(img.shape[1])
        seq = self.num_views
        r = self.raster
        if r.num_faces == 0:
            _host_f32("intrinsics", intrinsics, (3, 3))
            _host_f32("extrinsics", extrinsics, (4, 4))
            self.num_views += 1
            self.last_cos = torch.empty(0, dtype=torch.float32, device=self.device)
            return BakeStats(torch.tensor([0.0, 0.0, 0.0, float("nan")], dtype=torch.float64, device=self.device))
        visible = r.visible_faces(r.rasterize(intrinsics, extrinsics, H, W))
        self.num_views += 1        # a view that fails the check below still uses its number up: its stamps can never match again
        cos = self.select(visible, extrinsics, seq)
        self.last_cos = cos
        mean = self._mean_cos(cos, visible)
        if strict and float(mean) >= 0:          # the read-back; nothing has been baked yet, as in the script
            raise ValueError(f"The view direction is not correct. cos_angles.mean()={float(mean)}")
        self.sample(img, intrinsics, extrinsics, seq)
        limit = torch.tensor(COS_LIMIT, dtype=torch.float32, device=self.device)
        raw = torch.stack([visible.sum().to(torch.float64), (cos < limit).sum().to(torch.float64),
                           (self.baked_by == seq).sum().to(torch.float64), mean.to(torch.float64)])
        return BakeStats(raw)

    @staticmethod
    def _mean_cos(cos, visible):
        """cos_angles.mean() over the visible faces (NaN when there is none, or when one of them is degenerate)."""
        return torch.where(visible, cos, torch.zeros_like(cos)).sum() / visible.sum()


def bake_vertex_colors(vertices, faces, views, sampling="reference", strict=True):
    """texture_mesh.py's loop: views is a sequence of (image, intrinsics, extrinsics), baked in order, so that a vertex keeps
    the colour of the LAST view that sees it.  Returns (vertex_colors [V,3] float32, baked_by [V] int32: that view's position
    in `views`, -1 where no view baked the vertex (its colour is 0), [BakeStats per view])."""
    baker = TextureBaker(vertices, faces, sampling)
    stats = [baker.add_view(image, K, E, strict=strict) for image, K, E in views]
    return baker.vertex_colors, baker.baked_by, stats
