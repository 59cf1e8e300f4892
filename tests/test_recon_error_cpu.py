"""Reconstruction-error metric without a GPU: the latitude weights, the argument checks of the public entry point and
of the C ABI launcher (CRA5_ERR_ARG before any device work)."""
import numpy as np
import pytest
import torch

from cra5_amd import _lib, metrics, ops


def test_latitude_weights_era5_grid():
    w = metrics.latitude_weights(721)
    assert w.dtype == np.float64 and w.shape == (721,)
    assert abs(w.mean() - 1.0) <= 1e-15
    np.testing.assert_allclose(w, w[::-1], rtol=0, atol=1e-15)
    assert w[0] < 1e-15 and w[-1] < 1e-15
    assert w[360] == w.max()
    phi = np.deg2rad(90.0 - 180.0 * np.arange(721, dtype=np.float64) / 720.0)
    ref = np.cos(phi) / np.mean(np.cos(phi))
    np.testing.assert_array_equal(w, ref)


def test_latitude_weights_need_two_rows():
    assert metrics.latitude_weights(2).shape == (2,)
    for H in (1, 0):
        with pytest.raises(ValueError):
            metrics.latitude_weights(H)


def test_reconstruction_error_refuses_host_tensors_and_mismatched_shapes():
    x = torch.zeros((2, 3, 8))
    with pytest.raises(TypeError):
        metrics.reconstruction_error(x, x)                      # host tensors: the GPU is the only path
    with pytest.raises(TypeError):
        metrics.reconstruction_error(x.numpy(), x.numpy())
    with pytest.raises(TypeError):
        metrics.reconstruction_error(x.double(), x.double())
    with pytest.raises(TypeError):
        ops.recon_error(x, x)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.reconstruction_error(x, torch.zeros((2, 3, 9)))
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.reconstruction_error(x.unsqueeze(0), x)


def test_recon_error_abi_validates_arguments():
    L = _lib.lib()
    assert L.cra5_recon_error_f32(None, None, 1, 1, 1, None, None, 0, None, None) == -7
    nb = L.cra5_recon_error_slab_bytes(268, 721, 1440)
    assert nb > 0 and nb % (8 * 6) == 0
    assert L.cra5_recon_error_slab_bytes(0, 721, 1440) == 0
    assert L.cra5_recon_error_slab_bytes(1, -1, 4) == 0
    assert L.cra5_recon_error_slab_bytes(1, 1 << 16, 1 << 16) == 0          # H * W >= 2^31
    fake = 1 << 20   # (never dereferenced: every call below fails its checks before a launch)
    assert L.cra5_recon_error_f32(fake, fake, 0, 721, 1440, None, fake, nb, fake, None) == -7
    assert L.cra5_recon_error_f32(fake, fake, 268, 721, 1440, None, None, nb, fake, None) == -7
    assert L.cra5_recon_error_f32(fake, fake, 268, 721, 1440, None, fake, nb, None, None) == -7
    assert L.cra5_recon_error_f32(None, fake, 268, 721, 1440, None, fake, nb, fake, None) == -7
    assert L.cra5_recon_error_f32(fake, fake, 268, 721, 1440, None, fake, nb - 8, fake, None) == -7   # slab too small
