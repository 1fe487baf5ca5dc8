"""-m gpu: forward parity of the HIP path (through the C ABI) against the CPU oracle -- BIT-EXACT.

The oracle (oracle/gsr_oracle.c) restates $RAST/cuda_rasterizer/forward.cu + rasterizer_impl.cu with a
pinned FMA contraction and an explicit exp(); the HIP kernels implement the same arithmetic, so every
float of every output and intermediate must be identical (tolerance: 0 ulp; the north-star tolerance
of 1e-5 abs on RGB/depth applies to the comparison with the reference binary, tests/test_gpu_ref.py).
"""
import numpy as np
import pytest
import torch

from gaustudio_amd import scenes

from util import compare_forward_exact, hip_forward, oracle_forward, scene_kwargs, to_np

pytestmark = pytest.mark.gpu


def _run(oracle, P, W, H, D, use_sh=True, use_cov=False, seed=0, scale_modifier=1.0, sigma_px=1.5, bg=None):
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(P, cam, seed=seed, sigma_px_median=sigma_px)
    kw = scene_kwargs(sc, use_sh, use_cov)
    os_ = oracle_forward(oracle, sc, cam, D, kw, scale_modifier, bg)
    hs = hip_forward(sc, cam, D, kw, scale_modifier, bg)
    compare_forward_exact(hs, os_)
    return hs, os_


@pytest.mark.parametrize("D", [0, 1, 2, 3])
def test_c1_10k_400x400(oracle, D):
    """BASELINE config C1 (10k Gaussians, 400x400), every SH degree."""
    hs, os_ = _run(oracle, 10000, 400, 400, D)
    assert hs["num_rendered"] > 10000


@pytest.mark.parametrize("W,H", [(401, 399), (16, 16), (17, 33), (1, 1), (640, 8)])
def test_ragged_image_sizes(oracle, W, H):
    """Partial last tile row/column (1080 = 67.5 tiles in C3) and degenerate images."""
    _run(oracle, 3000, W, H, 3, seed=5, sigma_px=2.5)


def test_precomputed_colors_and_cov(oracle):
    _run(oracle, 5000, 320, 240, 0, use_sh=False, use_cov=False, seed=2)
    _run(oracle, 5000, 320, 240, 3, use_sh=True, use_cov=True, seed=3)
    _run(oracle, 5000, 320, 240, 0, use_sh=False, use_cov=True, seed=4)


def test_scale_modifier_and_white_bg(oracle):
    # out_color is NOT blended with bg in this fork, so white bg must not change the image
    a, _ = _run(oracle, 4000, 256, 256, 2, seed=7, scale_modifier=1.7)
    b, _ = _run(oracle, 4000, 256, 256, 2, seed=7, scale_modifier=1.7, bg=torch.ones(3))
    assert torch.equal(a["color"], b["color"])


def test_trailing_chunks_do_not_read_past_the_geometry_buffer(oracle):
    """the chunked binning kernels are launched with G chunks of roundup1024(ceil(P / G)) Gaussians, so for P just
    above G * 1024 the trailing chunks start behind the last Gaussian (base up to ~2 P); their culled lanes used to read
    `recs[base]`, up to ~5 MB past the geometry buffer.  P in (262144, ~309 k] for any T, (524288, ~619 k] when 4 T <= 72 KiB.
    Run under a non-caching allocator (each buffer its own hipMalloc) and checked against the oracle bit for bit."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTORCH_NO_CUDA_MEMORY_CACHING="1", GSR_FAST_EXP="0")
    r = subprocess.run([sys.executable, os.path.join(here, "guard_forward.py"), "262145x320x200", "300000x320x200", "524289x256x160",
                        "262145x2048x1200"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.count("ok ") == 4, (r.stdout[-1500:], r.stderr[-3000:])


def test_large_footprints_cooperative_binning(oracle):
    """Screen-filling Gaussians exercise the wave-cooperative tile walk (> 32 tiles per Gaussian)."""
    hs, os_ = _run(oracle, 600, 512, 384, 1, seed=11, sigma_px=60.0)
    assert int(to_np(hs["tiles_touched"]).max()) > 32


@pytest.mark.parametrize("P,lo,hi", [(2500, 256, 4096), (12000, 4096, 16384), (100000, 16384, 1 << 19), (700000, 1 << 19, 1 << 30)])
def test_long_tile_lists_lds_and_global_sort(oracle, P, lo, hi):
    """Per-tile lists in each regime of the sort: 2 k keys (past the 1024-key register network: one workgroup per list),
    10 k and 87 k keys per tile (queue pipeline: 2 and 11 slices per list, sample splitters, buckets of ~128), 600 k keys
    per tile (73 slices; the 512 buckets of the first cut hold ~1200 keys each: every one of them goes through
    segment_partition's second cut)."""
    cam = scenes.make_camera(48, 32)
    sc = scenes.make_scene(P, cam, seed=13, sigma_px_median=6.0)
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 0, kw)
    r = os_["ranges"]
    assert lo < int((r[:, 1] - r[:, 0]).max()) <= hi
    hs = hip_forward(sc, cam, 0, kw)
    compare_forward_exact(hs, os_)


def test_one_list_of_millions_of_keys(oracle):
    """One tile, 4.7 M keys: every one of the first cut's 512 buckets holds ~9 k keys, i.e. is a segment too long for a
    workgroup's registers -- segment_partition's streaming path (gs_partition_segment, n > 8192)."""
    cam = scenes.make_camera(16, 16)
    sc = scenes.make_scene(4_700_000, cam, seed=3, sigma_px_median=1.5)
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 0, kw)
    assert os_["ranges"].shape[0] == 1 and int(os_["ranges"][0, 1]) > 512 * 8192
    hs = hip_forward(sc, cam, 0, kw)
    compare_forward_exact(hs, os_)


def test_many_long_lists_and_a_giant_one(oracle):
    """The sort regime of a C4-like frame with one giant tile: more than 1024 lists beyond the one-wave sort (they take the
    one-workgroup-per-list kernel) AND lists beyond 8192 keys (the slice pipeline), in one frame."""
    cam = scenes.make_camera(576, 512)
    sc = scenes.make_scene(260000, cam, seed=21, sigma_px_median=5.0)
    m = sc.means3D.clone()
    K = 12000                                          # a clump on the line of sight of tile (10, 10), depths kept
    z = m[:K, 2]
    x = (10 * 16 + 8.5 - cam.width / 2) / (cam.width / 2) * cam.tanfovx
    y = (10 * 16 + 8.5 - cam.height / 2) / (cam.height / 2) * cam.tanfovy
    g = torch.Generator().manual_seed(5)
    m[:K, 0] = z * (x + 0.002 * torch.randn(K, generator=g))
    m[:K, 1] = z * (y + 0.002 * torch.randn(K, generator=g))
    sc = sc._replace(means3D=m.contiguous())
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 1, kw)
    n = os_["ranges"][:, 1].astype(np.int64) - os_["ranges"][:, 0]
    assert int((n > 1024).sum()) >= 1024 and int(n.max()) > 8192 and int((n <= 8192).sum()) > 1000
    hs = hip_forward(sc, cam, 1, kw)
    compare_forward_exact(hs, os_)


@pytest.mark.parametrize("P", [2000, 12000, 40000, 300000])
def test_depth_ties_resolve_by_id(oracle, P):
    """Equal depths inside a tile must order by ascending Gaussian id; P=12000: 3-6 k keys per tile, the
    one-workgroup-per-list kernel, whose equal-width depth buckets overflow on ~18 distinct depths: its counting-sort fallback
    with the per-run id fix-up; P=40000 puts ~10 k keys
    with only ~18 distinct depths in each tile (runs of ~500 equal depths), P=300000 ~75 k keys with runs of
    ~4 k: the radix path's long-run branch (full 64-bit LSD sort instead of the per-run fix-up)."""
    cam = scenes.make_camera(64, 64)
    sc = scenes.make_scene(P, cam, seed=17, sigma_px_median=4.0)
    means = sc.means3D.clone()
    z = torch.round(means[:, 2])          # only ~18 distinct depths
    means[:, 0] *= z / means[:, 2]
    means[:, 1] *= z / means[:, 2]
    means[:, 2] = z
    sc = sc._replace(means3D=means.contiguous())
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 3, kw)
    d = os_["depths"][os_["radii"] > 0]
    assert len(np.unique(d)) < 40
    hs = hip_forward(sc, cam, 3, kw)
    compare_forward_exact(hs, os_)


def test_all_culled_and_empty(oracle):
    from gaustudio_amd import _C
    cam = scenes.make_camera(100, 60)
    sc = scenes.make_scene(500, cam, seed=1)
    sc = sc._replace(means3D=(sc.means3D * torch.tensor([1.0, 1.0, -1.0])).contiguous())   # behind the camera
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 3, kw)
    assert os_["num_rendered"] == 0
    hs = hip_forward(sc, cam, 3, kw)
    assert hs["num_rendered"] == 0 and int(hs["radii"].abs().sum()) == 0
    for k in ("color", "depth", "median", "opacity"):
        assert np.array_equal(to_np(hs[k]), os_[k]), k
    # P == 0 (rasterize_points.cu:67-84): nothing is launched, the torch::full(0.0) images come back as they are
    # (all three median channels 0: the 15.0 sentinel only appears when the render kernel runs), rendered = 0
    e = torch.Tensor([])
    dev = "cuda"
    out = _C.rasterize_gaussians(torch.zeros(3), torch.zeros(0, 3, device=dev), e, torch.zeros(0, 1, device=dev),
                                 torch.zeros(0, 3, device=dev), torch.zeros(0, 4, device=dev), 1.0, e,
                                 cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.tanfovx, cam.tanfovy, cam.height,
                                 cam.width, torch.zeros(0, 16, 3, device=dev), 3, cam.campos.to(dev), False, False)
    assert out[0] == 0 and out[1].shape == (3, 60, 100) and float(out[1].abs().sum()) == 0.0
    assert float(out[3].abs().sum()) == 0.0 and float(out[2].abs().sum()) == 0.0 and float(out[4].abs().sum()) == 0.0
    assert out[5].numel() == 0


def test_mark_visible(oracle):
    from gaustudio_amd import _C
    cam = scenes.look_at_camera(64, 64, (3.0, 1.0, -6.0), (0.0, 0.0, 0.0))
    sc = scenes.make_ball_scene(5000, radius=8.0, seed=3)
    ref = oracle.mark_visible(sc.means3D.numpy(), cam.viewmatrix.numpy(), cam.projmatrix.numpy())
    got = _C.mark_visible(sc.means3D.cuda(), cam.viewmatrix.cuda(), cam.projmatrix.cuda())
    assert got.dtype == torch.bool and np.array_equal(to_np(got), ref)
    assert 0 < ref.sum() < ref.size
    got2 = _C.mark_visible(sc.means3D.cuda(), cam.viewmatrix, cam.projmatrix)   # host-side matrices accepted
    assert torch.equal(got, got2)


def test_prefiltered_violation_raises():
    from gaustudio_amd import _C
    cam = scenes.make_camera(64, 64)
    sc = scenes.make_scene(100, cam, seed=1)
    sc = sc._replace(means3D=(sc.means3D * torch.tensor([1.0, 1.0, -1.0])).contiguous())
    with pytest.raises(RuntimeError, match="prefiltered"):
        hip_forward(sc, cam, 0, scene_kwargs(sc, True, False), prefiltered=True)


def test_inward_ring_camera_rotated_view(oracle):
    """Non-identity view matrices (C4-style ring cameras looking at a ball of Gaussians)."""
    sc = scenes.make_ball_scene(20000, radius=3.0, seed=5, sigma=0.03)
    for cam in scenes.ring_cameras(3, 320, 208, radius=8.0):
        kw = scene_kwargs(sc, True, False)
        os_ = oracle_forward(oracle, sc, cam, 3, kw)
        hs = hip_forward(sc, cam, 3, kw)
        compare_forward_exact(hs, os_)
        assert os_["num_rendered"] > 1000


def test_forward_is_deterministic():
    """Two runs are bit-identical although bin_scatter fills tile segments with atomics: the per-tile
    sort key (depth, id) is unique."""
    cam = scenes.make_camera(800, 800)
    sc = scenes.make_scene(300000, cam, seed=21)
    kw = scene_kwargs(sc, True, False)
    a = hip_forward(sc, cam, 3, kw)
    b = hip_forward(sc, cam, 3, kw)
    for k in ("color", "depth", "median", "opacity", "radii", "point_list", "final_T", "n_contrib"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("W,H,path", [(3840, 2160, "lds-histogram binning with a 127 KiB histogram (C5 resolution)"),
                                      (5120, 2880, "fallback: device-atomic binning, tile grid too large for LDS")])
def test_large_tile_grids_both_binning_paths(oracle, W, H, path):
    hs, os_ = _run(oracle, 30000, W, H, 1, seed=23, sigma_px=4.0)
    assert hs["num_rendered"] > 30000


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500])
def test_single_tile_list_lengths_around_the_sort_size_classes(oracle, P):
    """A 16x16 image is ONE tile; every Gaussian sits inside it, so the tile list has exactly P keys: the boundaries of
    the register sort's size classes (1, 2, 4, 8, 16 keys per lane) and the hand-over to the radix path at 1024."""
    cam = scenes.make_camera(16, 16)
    sc = scenes.make_scene(P, cam, seed=100 + P, sigma_px_median=2.5)
    means = sc.means3D.clone()
    means[:, 0] *= 0.5
    means[:, 1] *= 0.5                                       # well inside the frame
    # opaque enough that every Gaussian reaches alpha >= 1/255 at its nearest pixel: none is pruned by the tight binning
    sc = sc._replace(means3D=means.contiguous(), opacities=torch.full_like(sc.opacities, 0.9))
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 1, kw)
    assert os_["num_rendered"] == P and os_["num_binned"] == P and os_["ranges"].shape[0] == 1
    hs = hip_forward(sc, cam, 1, kw)
    compare_forward_exact(hs, os_)


@pytest.mark.parametrize("name,P,W,H,D", [("C2", 300_000, 800, 800, 3), ("C3", 1_000_000, 1920, 1080, 3),
                                            ("C3-D0", 1_000_000, 1920, 1080, 0), ("C4-view", 5_000_000, 1297, 840, 3),
                                            ("C5-view", 2_500_000, 3840, 2160, 3)])
def test_baseline_configs_bit_exact_vs_oracle(oracle, name, P, W, H, D):
    """BASELINE configs C2, the full-size headline C3 (SH degree 3 and 0) and one view of the C4 / C5 sizes (20 M
    instances, ~3.7 k per tile: the long-list sort; a 4K frame): every output and every intermediate of the HIP path
    equals the CPU oracle's to the bit -- not just within the 1e-5 of the north star."""
    hs, os_ = _run(oracle, P, W, H, D)
    assert hs["num_binned"] < hs["num_rendered"]          # the tight binning dropped instances, the images did not notice


def _with_options(**opts):
    from contextlib import contextmanager
    from gaustudio_amd import _C

    @contextmanager
    def cm():
        old = {k: _C.get_option(k) for k in opts}
        try:
            for k, v in opts.items():
                _C.set_option(k, v)
            yield
        finally:
            for k, v in old.items():
                _C.set_option(k, v)
    return cm()


@pytest.mark.parametrize("P,W,H,D", [(20000, 400, 400, 3), (1_000_000, 1920, 1080, 3)], ids=["small", "C3"])
def test_culling_and_tight_binning_change_no_bit(P, W, H, D):
    """A/B against the library's own un-optimised configuration: with the wave-level box cull and the pcut pre-test
    disabled (every wave evaluates every staged instance) and with the reference's square getRect binning, the images,
    radii and num_rendered are bit-identical -- the optimisations only remove work."""
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(P, cam, seed=0)
    kw = scene_kwargs(sc, True, False)
    a = hip_forward(sc, cam, D, kw)
    with _with_options(cull=0):
        b = hip_forward(sc, cam, D, kw)
    with _with_options(tight_binning=0):
        c = hip_forward(sc, cam, D, kw)
    with _with_options(tight_binning=0, cull=0):
        d = hip_forward(sc, cam, D, kw)
    assert c["num_binned"] == c["num_rendered"] == a["num_rendered"] and a["num_binned"] < a["num_rendered"]
    for other in (b, c, d):
        assert other["num_rendered"] == a["num_rendered"]
        for k in ("color", "depth", "median", "opacity", "radii", "final_T"):
            assert torch.equal(a[k], other[k]), k
    for k in ("point_list", "ranges", "n_contrib"):
        assert torch.equal(a[k], b[k]), k          # same binning, only the cull differs


@pytest.mark.parametrize("P,W,H,D,sig", [(20000, 400, 400, 3, None), (30000, 333, 217, 1, 6.0), (3000, 131, 77, 0, 25.0),
                                         (1_000_000, 1920, 1080, 3, None)], ids=["small", "odd", "wide", "C3"])
def test_forward_variants_agree_bit_for_bit(P, W, H, D, sig):
    """composite_fwd with per-quarter (4x4) instance lists (default) against the walk without any culling: every
    output and the per-pixel state are bit-identical (image sizes that are not multiples of 16 or 4 included:
    clipped quarters)."""
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(P, cam, seed=1, **({} if sig is None else {"sigma_px_median": sig}))
    kw = scene_kwargs(sc, True, False)
    a = hip_forward(sc, cam, D, kw)
    with _with_options(cull=0):
        c = hip_forward(sc, cam, D, kw)
    for other in (c,):
        for k in ("color", "depth", "median", "opacity", "radii", "final_T", "n_contrib", "point_list", "ranges"):
            assert torch.equal(a[k], other[k]), k


def _adversarial_scene(P, cam, seed, kind):
    """Scenes aimed at the conservative block culls (gs_quarter_mask / gs_tight_rect): needles
    (axis ratios up to 1:300, every orientation), pancakes seen edge-on, screen-filling blobs, opacities hugging the
    1/255 visibility threshold and the 0.99 alpha clamp, and centres sitting on block and tile borders."""
    g = torch.Generator().manual_seed(seed)
    sc = scenes.make_scene(P, cam, seed=seed, sigma_px_median=4.0)
    scales, opac, means = sc.scales.clone(), sc.opacities.clone(), sc.means3D.clone()
    if kind == "needles":
        scales[:, 0] *= torch.exp(torch.rand(P, generator=g) * 5.7)            # up to x300 along one axis
        scales[:, 1] *= 0.2
    elif kind == "pancakes":
        scales[:, 2] *= 0.003
        scales[:, :2] *= 4.0
    elif kind == "blobs":
        scales *= torch.exp(torch.rand(P, 1, generator=g) * 4.0)               # up to x55: many tiles per Gaussian
    elif kind == "threshold":
        u = torch.rand(P, 1, generator=g)
        opac = torch.where(u < 0.5, 1.0 / 255.0 * (0.9 + 0.4 * torch.rand(P, 1, generator=g)),   # 0.9 .. 1.3 / 255
                           1.0 - 0.02 * torch.rand(P, 1, generator=g))                           # 0.98 .. 1.0
    elif kind == "borders":
        # snap the projected centres onto multiples of 4 pixels (+- half a pixel): block and tile borders
        z = means[:, 2]
        fx, fy = cam.width / (2 * cam.tanfovx), cam.height / (2 * cam.tanfovy)
        px = means[:, 0] / z * fx + cam.width / 2 - 0.5
        py = means[:, 1] / z * fy + cam.height / 2 - 0.5
        px = torch.round(px / 4) * 4 + (torch.randint(0, 3, (P,), generator=g) - 1) * 0.5
        py = torch.round(py / 4) * 4 + (torch.randint(0, 3, (P,), generator=g) - 1) * 0.5
        means[:, 0] = (px + 0.5 - cam.width / 2) / fx * z
        means[:, 1] = (py + 0.5 - cam.height / 2) / fy * z
    return sc._replace(scales=scales.contiguous(), opacities=opac.contiguous(), means3D=means.contiguous())


@pytest.mark.parametrize("kind", ["needles", "pancakes", "blobs", "threshold", "borders"])
def test_block_culls_are_conservative_on_adversarial_scenes(oracle, kind):
    """The per-quarter walk (default) and the walk without any culling give the same bits on scenes built to stress
    the culls; the default is also compared with the CPU oracle (which has no cull at all)."""
    W, H = 331, 203
    cam = scenes.make_camera(W, H)
    sc = _adversarial_scene(6000 if kind != "blobs" else 1500, cam, seed=31, kind=kind)
    kw = scene_kwargs(sc, True, False)
    a = hip_forward(sc, cam, 2, kw)
    with _with_options(cull=0):
        c = hip_forward(sc, cam, 2, kw)
    with _with_options(cull=0, tight_binning=0):
        d = hip_forward(sc, cam, 2, kw)
    for other in (c, d):
        for k in ("color", "depth", "median", "opacity", "radii", "final_T"):
            assert torch.equal(a[k], other[k]), (kind, k)
    compare_forward_exact(a, oracle_forward(oracle, sc, cam, 2, kw))


def test_speculative_launch_overflow_is_retried():
    """The kernels behind the instance count are enqueued against the remembered binning capacity before the host
    has read the count; when the capacity is too small (forced here) they leave without touching memory and the host
    re-allocates and re-launches.  Results must be those of the ordinary path; so must a capacity that is too small
    only for the long-list sort (a tile list > 1024 keys after a frame without one)."""
    from gaustudio_amd import _C
    cam = scenes.make_camera(320, 240)
    sc = scenes.make_scene(40000, cam, seed=3, sigma_px_median=2.5)
    kw = scene_kwargs(sc, True, False)
    with _with_options(speculative=0):
        want = hip_forward(sc, cam, 3, kw)
    _C.set_option("bin_capacity", 1000)                      # far below num_binned
    got = hip_forward(sc, cam, 3, kw)
    assert _C.get_option("bin_capacity") >= want["num_binned"]
    again = hip_forward(sc, cam, 3, kw)                      # now speculates successfully
    for g in (got, again):
        for k in ("color", "depth", "median", "opacity", "radii", "point_list", "ranges", "n_contrib", "final_T"):
            assert torch.equal(want[k], g[k]), k
    # a frame with a > 1024-key tile list right after frames without one: the speculative launch lacks the radix path
    cam2 = scenes.make_camera(48, 32)
    sc2 = scenes.make_scene(12000, cam2, seed=13, sigma_px_median=6.0)
    kw2 = scene_kwargs(sc2, True, False)
    with _with_options(speculative=0):
        want2 = hip_forward(sc2, cam2, 0, kw2)
    hip_forward(sc, cam, 3, kw)                              # resets the "long lists" memory
    got2 = hip_forward(sc2, cam2, 0, kw2)
    for k in ("color", "depth", "median", "opacity", "point_list", "n_contrib"):
        assert torch.equal(want2[k], got2[k]), k


def test_device_selftest():
    """v_rcp_f32(1.0) == 1.0 on this device: composite_bwd carries dead pixels through without a select on T."""
    from gaustudio_amd import _C
    assert _C.selftest() == 3


def test_clustered_scene_bit_exact_vs_oracle(oracle):
    """The NON-UNIFORM bench workload (bench.py --workload C2-clustered: 300 k Gaussians in 48 clusters, inward ring camera,
    36 % empty tiles, per-tile lists p50 ~ 10 / p99 ~ 11 k / max ~ 58 k, 1 % of the splats 50-60 px wide): forward bit-exact
    against the CPU oracle (every sort regime and the empty-tile path in one frame), backward inside the summation bound."""
    from test_gpu_backward import _check
    W = H = 800
    sc = scenes.make_clustered_scene(300_000, W, cam_distance=11.0, seed=0)
    cam = scenes.ring_cameras(5, W, H, radius=11.0)[1]
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 3, kw)
    hs = hip_forward(sc, cam, 3, kw)
    compare_forward_exact(hs, os_)
    r = os_["ranges"]
    n = r[:, 1].astype(np.int64) - r[:, 0].astype(np.int64)
    assert (n == 0).mean() > 0.2 and n.max() > 20 * n.mean() and n.max() > 16384
    _check(oracle, sc, cam, 3, kw)


@pytest.mark.parametrize("view", [0, 3])
def test_c4_inside_view_bit_exact_vs_oracle(oracle, view):
    """The C4-inside bench workload (bench.py --workload C4-inside; VERDICT r4 #3: BASELINE config 4 is a 360-degree capture, the
    cameras stand INSIDE the scene) at reduced P: a ball of radius 6, ring cameras at radius 2.5 looking through the centre, one
    1297x840 view.  A view sees ~16 % of the Gaussians (the others are behind the camera or outside the frustum), Gaussians next to
    the camera cover hundreds of pixels: forward bit-exact against the CPU oracle, backward inside the summation bound."""
    from test_gpu_backward import _check
    W, H, P = 1297, 840, 400_000
    sc = scenes.make_ball_scene(P, radius=6.0, seed=0, sigma=0.008)
    cam = scenes.ring_cameras(8, W, H, radius=2.5)[view]
    kw = scene_kwargs(sc, True, False)
    os_ = oracle_forward(oracle, sc, cam, 3, kw)
    hs = hip_forward(sc, cam, 3, kw)
    compare_forward_exact(hs, os_)
    vis = float((os_["radii"] > 0).mean())
    assert 0.12 < vis < 0.20 and int(os_["radii"].max()) > 300, (vis, int(os_["radii"].max()))
    _check(oracle, sc, cam, 3, kw)


def test_inside_camera_late_sh_request_bit_exact(oracle):
    """Round 5: preprocess_fwd requests a Gaussian's 192-B SH row only once the Gaussian has turned out visible (rounds 2-4: right
    after the near-plane test -- a Gaussian in front of the camera but outside the image fetched it for nothing; the reference has
    no x / y frustum test, auxiliary.h:147-161).  A view from INSIDE a ball (84 % culled, half of them in front of the camera), also
    with unnormalised quaternions and a scale modifier, and footprints from sub-pixel to a third of the image: bit-identical to the
    oracle."""
    W, H = 640, 400
    sc = scenes.make_ball_scene(120_000, radius=6.0, seed=1, sigma=0.02)
    cam = scenes.ring_cameras(8, W, H, radius=2.5)[5]
    kw = scene_kwargs(sc, True, False)
    compare_forward_exact(hip_forward(sc, cam, 3, kw), oracle_forward(oracle, sc, cam, 3, kw))
    sc2 = sc._replace(rotations=(sc.rotations * torch.linspace(0.3, 3.0, sc.rotations.shape[0])[:, None]).contiguous())
    kw2 = scene_kwargs(sc2, True, False)
    compare_forward_exact(hip_forward(sc2, cam, 2, kw2, scale_modifier=2.5), oracle_forward(oracle, sc2, cam, 2, kw2, 2.5))
    _run(oracle, 20000, 333, 211, 3, seed=4, sigma_px=3.0)
    _run(oracle, 20000, 333, 211, 1, seed=5, sigma_px=40.0)
