"""TEST INFRASTRUCTURE shared by the surfel caller-pin generator (dev container, the reference's unmodified SurfelRenderer) and
the tests (any box): the surfel renderer cases, a RECORDING stand-in for `diff_surfel_rasterization`, and a restatement of
SurfelRenderer (gaustudio/renderers/surfel_renderer.py) that replays the same calls on a box without the reference checkout.

The restatement is PINNED by tests/golden/py_surfel_calls.json (tests/golden/make_surfel_call_fixture.py): given the same seeded
point cloud and the recording stand-in, `replay_case` must give the record the unmodified class gave."""
import math
import types

import torch

import render_call_record as rcr

# every case = one SurfelRenderer configuration (surfel_renderer.py:8-15) on a 2-scale point cloud (configs/2dgs.yaml: scale: 2)
CASES = [
    dict(name="surfel_train_deg3", renderer="surfel_renderer", config={}, model="vanilla2d", active_sh_degree=3, grad=True),
    dict(name="surfel_train_deg1_white_modifier", renderer="surfel_renderer",
         config={"white_background": True, "scaling_modifier": 1.3}, model="vanilla2d", active_sh_degree=1, grad=True),
    dict(name="surfel_convert_SHs_python", renderer="surfel_renderer", config={"convert_SHs_python": True}, model="vanilla2d",
         active_sh_degree=2, grad=True),
    dict(name="surfel_eval_no_grad", renderer="surfel_renderer", config={}, model="vanilla2d", active_sh_degree=3, grad=False,
         no_grad=True),
    # (compute_cov3D_python=True is not a case: with 2 stored scales GauStudio's own get_covariance fails before the operator is
    # called -- models/utils.py build_scaling_rotation indexes a third scale)
]

DEFAULTS = {"kernel_size": 0.0, "scaling_modifier": 1.0, "white_background": False, "convert_SHs_python": False,
            "compute_cov3D_python": False, "debug": False}       # surfel_renderer.py:8-15


def recording_module():
    """A module object exporting GaussianRasterizationSettings (the 12-field tuple) and a GaussianRasterizer that records its call
    and returns zeros of the surfel operator's output shapes: (color [3,H,W], radii [P] int32, allmap [7,H,W])."""
    from gaustudio_amd.surfel import GaussianRasterizationSettings
    mod = types.ModuleType("diff_surfel_rasterization")
    mod.calls = []

    class GaussianRasterizer(torch.nn.Module):
        def __init__(self, raster_settings):
            super().__init__()
            self.raster_settings = raster_settings

        def forward(self, *args, **kw):
            rs = self.raster_settings
            m3 = kw.get("means3D")
            rec = {"positional_args": len(args), "keywords": sorted(kw), "grad_enabled": torch.is_grad_enabled(),
                   "settings": {}, "arguments": {k: rcr.describe_tensor(v, m3) for k, v in kw.items()}}
            for f in rs._fields:
                v = getattr(rs, f)
                if torch.is_tensor(v):
                    rec["settings"][f] = {"tensor": rcr.describe_tensor(v, m3 if f != "bg" else None),
                                          "values": [float(x) for x in v.flatten().tolist()] if f == "bg" else None}
                else:
                    rec["settings"][f] = {"type": type(v).__name__, "value": v}
            mod.calls.append(rec)
            H, W = int(rs.image_height), int(rs.image_width)
            z = lambda *s: torch.zeros(*s, device=m3.device)
            return z(3, H, W), torch.zeros(m3.shape[0], dtype=torch.int32, device=m3.device), z(7, H, W)

    mod.GaussianRasterizationSettings = GaussianRasterizationSettings
    mod.GaussianRasterizer = GaussianRasterizer
    return mod


def comparable(call):
    """The part of a record that must be identical between the generator's run and a replay: everything but the fields that
    describe the box (see render_call_record.comparable)."""
    return rcr.comparable(call)


def renderer_state(config):
    conf = {**DEFAULTS, **config}
    bg = torch.tensor([1, 1, 1], dtype=torch.float32) if conf["white_background"] else torch.tensor([0, 0, 0], dtype=torch.float32)
    return bg, conf


def properties_like_reference(conf, raw, active_sh_degree, camera, max_sh_degree=3):
    """SurfelRenderer.get_gaussians_properties (surfel_renderer.py:27-47) with VanillaPointCloud's activations
    (models/vanilla_sg.py:27-37,58-63,102-106): -> (xyz, shs, colors_precomp, opacity, scales, rotations, cov3D_precomp)."""
    import caller_replay
    xyz = raw["xyz"]
    opacity = torch.sigmoid(raw["opacity"])
    scales = rotations = cov3D_precomp = None
    if conf["compute_cov3D_python"]:
        cov3D_precomp = caller_replay._covariance(torch.exp(raw["scale"]), conf["scaling_modifier"], raw["rot"])
    else:
        scales = torch.exp(raw["scale"])
        rotations = torch.nn.functional.normalize(raw["rot"])
    features = torch.cat((raw["f_dc"].reshape(len(raw["f_dc"]), -1, 3), raw["f_rest"].reshape(len(raw["f_dc"]), -1, 3)), dim=1)
    shs = colors_precomp = None
    if conf["convert_SHs_python"]:
        dir_pp = xyz - camera.camera_center.repeat(features.shape[0], 1)
        dir_n = dir_pp / dir_pp.norm(dim=1, keepdim=True)
        nc = (active_sh_degree + 1) ** 2
        sh2rgb = (caller_replay._sh_basis(dir_n, active_sh_degree)[:, :, None] * features[:, :nc]).sum(1)
        colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)
    else:
        shs = features
    return xyz, shs, colors_precomp, opacity, scales, rotations, cov3D_precomp


def render_like_surfel_renderer(props, camera, active_sh_degree, bg_color, scaling_modifier=1.0, debug=False, device="cuda",
                                Settings=None, Rasterizer=None):
    """SurfelRenderer.render (surfel_renderer.py:49-124), call for call, including the post-processing of the allmap."""
    if Settings is None:
        from diff_surfel_rasterization import GaussianRasterizationSettings as Settings, GaussianRasterizer as Rasterizer
    xyz, shs, colors_precomp, opacity, scales, rotations, cov3D_precomp = props
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=device) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:       # noqa: BLE001  (the reference's bare except)
        pass
    raster_settings = Settings(
        image_height=int(camera.image_height), image_width=int(camera.image_width),
        tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5),
        bg=bg_color.to(camera.world_view_transform.device), scale_modifier=scaling_modifier,
        viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform,
        sh_degree=active_sh_degree if shs is not None else 1, campos=camera.camera_center, prefiltered=False, debug=debug)
    rasterizer = Rasterizer(raster_settings=raster_settings)
    rendered_image, radii, allmap = rasterizer(means3D=xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
                                               opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    render_alpha = allmap[1:2]
    render_normal = allmap[2:5]
    render_normal = (render_normal.permute(1, 2, 0) @ (camera.world_view_transform[:3, :3].T)).permute(2, 0, 1)
    render_depth_median = torch.nan_to_num(allmap[5:6], 0, 0)
    render_depth_expected = torch.nan_to_num(allmap[0:1] / render_alpha, 0, 0)
    if len(allmap) > 7:
        rendered_median_weight, rendered_median_id = allmap[7:8], allmap[8:9].int()
    else:
        rendered_median_weight = rendered_median_id = None
    return {"render": rendered_image, "rendered_normal": render_normal, "rendered_depth": render_depth_expected,
            "rendered_median_depth": render_depth_median, "rendered_median_weight": rendered_median_weight,
            "rendered_median_id": rendered_median_id, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "rendered_final_opacity": render_alpha, "radii": radii}


def describe_package(pkg):
    return {k: (None if v is None else {"shape": list(v.shape), "dtype": str(v.dtype)}) for k, v in sorted(pkg.items())}


def generator_camera():
    """The camera of the generator: Camera(R = I, T = (0.1, -0.2, 4), FoV 60 x 40 degrees, 96 x 64)."""
    return dict(R_eye=True, T=(0.1, -0.2, 4.0), fovx=math.radians(60), fovy=math.radians(40), width=96, height=64)


def replay_case(case, device, Settings=None, Rasterizer=None):
    """One case replayed on `device`.  With the recording stand-in (default): -> (record, package, raw).  With the real operator
    (Settings / Rasterizer given): -> (None, package, raw)."""
    import numpy as np
    import caller_replay
    from gaustudio_amd import formats
    recording = Settings is None
    if recording:
        rec_mod = recording_module()
        Settings, Rasterizer = rec_mod.GaussianRasterizationSettings, rec_mod.GaussianRasterizer
    raw = rcr.raw_attributes(case, device)
    g = generator_camera()
    c = formats.CameraRecord(0, "replay", g["width"], g["height"], np.eye(3), np.array(g["T"]), g["fovx"], g["fovy"]).cam
    view = c.viewmatrix.t().contiguous().t()            # datasets/__init__.py: a transposed view, a sliced camera centre
    campos = torch.inverse(view)[3][:3]
    cam = caller_replay.Camera(g["width"], g["height"], g["fovx"], g["fovy"], view.to(device), c.projmatrix.to(device), campos.to(device))
    bg, conf = renderer_state(case["config"])
    with torch.set_grad_enabled(not case.get("no_grad", False)):
        props = properties_like_reference(conf, raw, case["active_sh_degree"], cam)
        pkg = render_like_surfel_renderer(props, cam, case["active_sh_degree"], bg, conf["scaling_modifier"], conf["debug"],
                                          device=device, Settings=Settings, Rasterizer=Rasterizer)
    if not recording:
        return None, pkg, raw
    assert len(rec_mod.calls) == 1
    call = rec_mod.calls[0]
    call["returns"] = describe_package(pkg)
    return call, pkg, raw
