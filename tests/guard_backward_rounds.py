"""Run as a script by tests/test_gpu_backward_rounds.py::test_every_lane_loads_inside_the_buffers_under_a_non_caching_allocator, in a
process whose torch allocator does not cache (PYTORCH_NO_CUDA_MEMORY_CACHING=1: every opaque buffer is its own hipMalloc, nothing
of this process sits behind it): composite_bwd's staging loads are issued by every lane, clamped into the tile's list, and must stay
inside the binning and geometry buffers where those are smallest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import gaustudio_amd
    from gaustudio_amd import scenes
    from oracle import pyoracle as po   # checker
    from test_gpu_backward import _check
    from test_gpu_backward_rounds import _saturated, _splats, _tile_stats
    from util import oracle_forward, scene_kwargs
    po.build()

    def run(name, sc, cam, **opts):
        kw = scene_kwargs(sc, True, False)
        os_ = oracle_forward(po, sc, cam, 1, kw)
        with gaustudio_amd.options(**opts):
            _check(po, sc, cam, 1, kw, seed=1)
        torch.cuda.synchronize()
        length, _ = _tile_stats(os_, cam)
        print(f"ok {name} binned={os_['num_binned']} tiles={len(length)} empty={int((length == 0).sum())}", flush=True)
        return os_, length

    # a frame most of whose tiles are empty: three small splats in the first tile of a 4x3-tile image
    cam = scenes.make_camera(64, 48)
    small = scenes.make_camera(16, 16)
    sc = _splats(small, 3, sigma_px=1.0, opacity=0.5, z_lo=3.0, z_hi=4.0, seed=1)
    sc = sc._replace(means3D=(sc.means3D * torch.tensor([0.2, 0.2, 1.0]) - torch.tensor([1.2, 0.9, 0.0])).contiguous())
    os_, length = run("empty-tiles", sc, cam)
    assert (length == 0).sum() >= 6 and os_["num_binned"] > 0
    # one to three binned instances in a one-tile frame
    for n in (1, 2, 3):
        os_, _ = run(f"binned-{n}", _splats(small, n, sigma_px=3.0, opacity=0.5, z_lo=3.0, z_hi=4.0, seed=n), small)
        assert os_["num_binned"] == n
    # the same without the forward's block masks, and a dead tail behind a saturated tile (two trips of the zero-rows loop)
    run("no-masks", _splats(small, 2, sigma_px=3.0, opacity=0.5, z_lo=3.0, z_hi=4.0, seed=7), small, cull=False)
    sc, _, _ = _saturated(po, small, 257, seed=257)
    run("dead-tail", sc, small)


if __name__ == "__main__":
    main()
