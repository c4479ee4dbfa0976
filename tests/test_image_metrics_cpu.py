"""Host side of the image metrics (no GPU): the workspace query, the tile query and the refusal of CPU tensors."""
import ctypes

import pytest
import torch


def test_workspace_bytes_monotone():
    from nerf_amd._lib import lib
    L = lib()
    q = L.nerf_image_metrics_workspace_bytes
    assert q(1, 11, 11) > 0
    for n, h, w in ((1, 11, 11), (3, 42, 43), (2, 75, 75), (1, 800, 800)):
        base = q(n, h, w)
        assert base > 0
        assert q(n + 1, h, w) >= base
        for d in (1, 31, 32, 33, 100):
            assert q(n, h + d, w) >= base
            assert q(n, h, w + d) >= base
    # the partials of 2^31 / 3 pixels' worth of images still fit the int64 result
    assert q(1 << 20, 800, 800) > q(1 << 19, 800, 800) > 0
    assert q(1, 10, 800) == -1 and q(1, 800, 10) == -1 and q(-1, 800, 800) == -1


def test_tile_is_positive():
    from nerf_amd._lib import lib
    from nerf_amd import kernels as K
    th, tw = K.image_metrics_tile()
    assert th > 0 and tw > 0
    assert lib().nerf_image_metrics_tile(None, ctypes.byref(ctypes.c_int(0))) == -1


def test_image_metrics_refuses_cpu_tensors():
    from nerf_amd import kernels as K, metrics
    a = torch.zeros(16, 16, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.image_metrics(a, a)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.image_metrics(a, a.to(torch.uint8), "srgb")
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.image_metrics(a, a)


def test_image_ssim_is_exported():
    from nerf_amd import losses
    assert callable(losses.image_ssim) and callable(losses.image_psnr)
