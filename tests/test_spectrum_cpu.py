"""Zonal power spectra without a GPU: the float64 reference of the tests against closed forms and Parseval, the host-side
resolved wavenumber, and the argument checks of the public entry points and of the C ABI launcher (CRA5_ERR_ARG before
any device work)."""
import numpy as np
import pytest
import torch

from cra5_amd import _lib, metrics, ops
from spectrum_helpers import ref_spectrum, smooth_pair, weights32, zonal_power


def lat_cases(H):
    return [None, metrics.latitude_weights(H), np.linspace(0.5, 1.5, H)]


@pytest.mark.parametrize("W", [1440, 240, 45, 2])
def test_reference_closed_forms(W):
    H, K = 7, W // 2 + 1
    w = np.arange(W, dtype=np.float64)
    for lat in lat_cases(H):
        L = weights32(lat, H)
        # a constant: all of it in k = 0
        p = zonal_power(np.full((1, H, W), 3.5), L)[0]
        assert abs(p[0] - 3.5 ** 2 * L.mean()) <= 1e-14 * p[0]
        assert np.all(np.abs(p[1:]) <= 1e-28 * p[0])
        # a single harmonic: a^2 mean(L) / 2 in its bin, a^2 mean(L) cos^2(phi) at the Nyquist bin of an even W
        for k0 in sorted({1, 7, W // 2} & set(range(1, K))):
            a, phi = 2.5, 0.3
            f = a * np.cos(2.0 * np.pi * k0 * w / W + phi)
            p = zonal_power(np.broadcast_to(f, (1, H, W)).copy(), L)[0]
            want = a * a * L.mean() * (np.cos(phi) ** 2 if 2 * k0 == W else 0.5)
            assert abs(p[k0] - want) <= 1e-13 * want, (W, k0)
            rest = np.delete(p, k0)
            assert np.all(np.abs(rest) <= 1e-26 * want), (W, k0)
        if W % 2 == 0:   # phase 0 at the Nyquist bin: the full a^2 mean(L)
            f = 2.5 * np.cos(np.pi * w)
            p = zonal_power(np.broadcast_to(f, (1, H, W)).copy(), L)[0]
            assert abs(p[W // 2] - 2.5 ** 2 * L.mean()) <= 1e-13 * p[W // 2]


@pytest.mark.parametrize("shape", [(2, 9, 45), (2, 5, 240), (1, 3, 1440), (1, 2, 2)])
def test_reference_parseval(shape):
    C, H, W = shape
    xh, x = smooth_pair(C, H, W, seed=W)
    for lat in lat_cases(H):
        L = weights32(lat, H)
        r = ref_spectrum(xh, x, lat)
        d = (xh - x).astype(np.float64)
        for name, f in (("power_truth", x.astype(np.float64)), ("power_recon", xh.astype(np.float64)), ("power_error", d)):
            want = (L[None, :, None] * f * f).mean(axis=(1, 2))
            assert np.all(np.abs(r[name].sum(axis=1) - want) <= 1e-13 * want), name
        assert r["wavenumber"].tolist() == list(range(W // 2 + 1)) and r["nonfinite"].tolist() == [0] * C


def test_reference_nonfinite_rule_and_resolved_wavenumber():
    xh, x = smooth_pair(3, 4, 30, seed=1)
    clean = ref_spectrum(xh, x, None)
    xh[1, 2, 3] = np.nan
    x[1, 2, 3] = np.inf
    x[1, 0, 0] = -np.inf
    r = ref_spectrum(xh, x, None)
    assert r["nonfinite"].tolist() == [0, 2, 0] and r["resolved_wavenumber"][1] == -1
    for name in ("power_truth", "power_recon", "power_error"):
        assert np.isnan(r[name][1]).all()
        assert np.array_equal(r[name][[0, 2]], clean[name][[0, 2]])
    # the package's host-side rule: the first k >= 1 with error >= truth, K if none, -1 for a flagged channel
    pt = np.array([[9.0, 4.0, 2.0, 1.0], [9.0, 4.0, 2.0, 1.0], [0.0, 4.0, 2.0, 1.0], [np.nan] * 4])
    pe = np.array([[10.0, 1.0, 2.0, 5.0], [1.0, 1.0, 1.0, 0.5], [5.0, 4.0, 0.0, 0.0], [np.nan] * 4])
    got = metrics.resolved_wavenumber(pt, pe, np.array([0, 0, 0, 3]))
    assert got.dtype == np.int64 and got.tolist() == [2, 4, 1, -1]      # (k = 0 never counts)
    assert np.array_equal(r["resolved_wavenumber"], metrics.resolved_wavenumber(r["power_truth"], r["power_error"], r["nonfinite"]))


def test_supported_widths():
    assert ops.SPECTRUM_MAX_W >= 1440
    good = [2, 3, 4, 5, 30, 45, 96, 120, 240, 288, 360, 480, 720, 1440,      # 1440 / k for every coarsen k among them
            729, 1125, 1215]                                                 # odd and above 720: twiddles from the global table
    bad = [0, 1, 7, 44, 1439, ops.SPECTRUM_MAX_W + 1, 2 * 1440, 7 * 128]
    assert all(ops.spectrum_width_ok(W) for W in good) and not any(ops.spectrum_width_ok(W) for W in bad)
    L = _lib.lib()
    for W in good:
        assert L.cra5_zonal_spectrum_slab_bytes(2, 5, W) > 0, W
    for W in bad:
        assert L.cra5_zonal_spectrum_slab_bytes(2, 5, W) == 0, W


def test_transform_helpers_on_the_host(tmp_path):
    """The kernel's own pass / twiddle / unpack code, compiled for the host and run thread by thread against a long-double
    DFT (tests/spectrum_host_check.hip): every radix mix, both twiddle-table forms, odd widths above 720 included."""
    import os
    import subprocess
    from cra5_amd import build as B
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spectrum_host_check.hip")
    exe = str(tmp_path / "spectrum_host_check")
    subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "W 1215" in r.stdout and "W 1440" in r.stdout


def test_zonal_spectrum_abi_validates_arguments():
    L = _lib.lib()
    f = L.cra5_zonal_spectrum_f32
    assert f(None, None, 1, 1, 2, None, None, None, 0, None, None, None) == -7
    nb = L.cra5_zonal_spectrum_slab_bytes(268, 721, 1440)
    assert nb > 0 and nb % 8 == 0 and nb % (3 * 721 + 1) == 0
    fake = 1 << 20   # (never dereferenced: every call below fails its checks before a launch)
    for i in (0, 1, 6, 7, 9, 10):       # x_hat, x, twiddle, slab, out, nonfinite
        a = [fake, fake, 268, 721, 1440, None, fake, fake, nb, fake, fake, None]
        a[i] = None
        assert f(*a) == -7, i
    for C, H, W in [(0, 721, 1440), (268, 0, 1440), (268, 721, 44), (268, 721, 7), (268, 721, ops.SPECTRUM_MAX_W + 1),
                    (268, 721, 2048), (268, 721, 1), (268, 721, 0), (1, 1 << 21, 1024), (1 << 16, 2, 4)]:
        assert L.cra5_zonal_spectrum_slab_bytes(C, H, W) == 0, (C, H, W)
        assert f(fake, fake, C, H, W, None, fake, fake, nb, fake, fake, None) == -7, (C, H, W)
    assert f(fake, fake, 268, 721, 1440, None, fake, fake, nb - 8, fake, fake, None) == -7     # slab one element short
    assert f(fake + 2, fake, 268, 721, 1440, None, fake, fake, nb, fake, fake, None) == -7     # misaligned frame


def test_zonal_spectrum_refuses_host_tensors_and_mismatched_shapes():
    x = torch.zeros((2, 3, 8))
    with pytest.raises(TypeError):
        metrics.zonal_spectrum(x, x)                      # host tensors: the GPU is the only path
    with pytest.raises(TypeError):
        metrics.zonal_spectrum(x.numpy(), x.numpy())
    with pytest.raises(TypeError):
        metrics.zonal_spectrum(x.double(), x.double())
    with pytest.raises(TypeError):
        ops.zonal_spectrum(x, x)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.zonal_spectrum(x, torch.zeros((2, 3, 9)))
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.zonal_spectrum(x.unsqueeze(0), x)
