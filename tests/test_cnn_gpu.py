"""the CNN zoo codecs (bmshj2018-factorized / -hyperprior, mbt2018-mean) on the HIP
kernels against golden vectors produced by the REFERENCE's own classes
(cra5/models/compressai/models/google.py:64-508; tests/golden/make_golden.py --stage cnn)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cra5_amd import cnn, synth

gpu = pytest.mark.gpu
N, M = 32, 48


def rel(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1)
    b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / torch.sqrt(torch.mean(b ** 2)))


def sub(t, step):
    return t.detach().reshape(-1)[::step].cpu()


@gpu
@pytest.mark.parametrize("name,cls", [("factorized", cnn.FactorizedPrior), ("hyperprior", cnn.ScaleHyperprior),
                                      ("meanscale", cnn.MeanScaleHyperprior)])
def test_cnn_zoo_vs_reference_golden(dev, golden_dir, name, cls, ledger):
    g = np.load(f"{golden_dir}/cnn_zoo.npz")
    keys = json.load(open(f"{golden_dir}/state_keys.json"))["cnn"][name]
    net = cls(N, M)
    synth.load_synthetic(net, seed=11)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == keys        # same module tree / buffers / tables
    net = net.to(dev)
    x = torch.from_numpy(g["x"]).to(dev)
    y = net.g_a(x[0])
    e_y = rel(y, g[f"{name}_y"])
    fw = net(x)
    e_fw = rel(sub(fw["x_hat"], 5), g[f"{name}_xhat_fw"])
    gy = torch.Generator().manual_seed(5)
    y_hat = torch.round(3.0 * torch.randn((1,) + tuple(y.shape), generator=gy))[0].to(dev)
    e_dec = rel(sub(net.g_s(y_hat), 5), g[f"{name}_xhat_synth"])
    print(f"{name}: y rel {e_y:.2e}, forward x_hat rel {e_fw:.2e}, decoder (given y_hat) rel {e_dec:.2e}")
    assert e_y <= 1e-5 and e_dec <= 1e-5
    assert e_fw <= 1e-3          # forward() rounds y: a .5-boundary flip moves x_hat locally, not globally
    for k, v in fw["likelihoods"].items():
        bits = float((-torch.log2(v.double())).sum())
        assert abs(bits - g[f"{name}_bits_{k}"][0]) <= 2e-3 * g[f"{name}_bits_{k}"][0], k
    if name != "factorized":
        z = net.h_a(net._h_a_in(y))
        assert rel(z, g[f"{name}_z"]) <= 1e-5
    # entropy coding: streams byte-identical to the reference python's when the integer side agrees,
    # decode(encode(x)) reproduces the forward pass' quantised reconstruction either way
    out = net.compress(x)
    assert list(out["shape"]) == list(g[f"{name}_shape"])
    same = [out["strings"][i][0] == g[f"{name}_string{i}"].tobytes() for i in range(len(out["strings"]))]
    lens = [(len(out["strings"][i][0]), len(g[f"{name}_string{i}"])) for i in range(len(out["strings"]))]
    print(f"{name}: streams identical to the reference python's: {same} (bytes {lens})")
    for (a, b) in lens:
        assert abs(a - b) <= 16
    rec = net.decompress(out["strings"], out["shape"])["x_hat"]
    assert rec.shape == x.shape
    assert rel(sub(rec, 5), g[f"{name}_xhat_rt"]) <= 1e-3
    if all(same):
        assert rel(sub(rec, 5), g[f"{name}_xhat_rt"]) <= 1e-5
        ledger.ran(f"cnn {name}: streams == reference-python-written streams, round trip <= 1e-5", f"bytes {lens}")
    else:
        ledger.not_applicable(f"cnn {name}: streams == reference-python-written streams", f"identical per stream: {same}")
    # ... and decoding the REFERENCE's streams gives the reference's reconstruction
    ref_strings = [[g[f"{name}_string{i}"].tobytes()] for i in range(len(out["strings"]))]
    if all(same) or name == "factorized":
        rec2 = net.decompress(ref_strings, out["shape"])["x_hat"]
        assert rel(sub(rec2, 5), g[f"{name}_xhat_rt"]) <= 1e-5
        ledger.ran(f"cnn {name}: reference-python-written streams decode to the reference's reconstruction")
    else:
        ledger.not_applicable(f"cnn {name}: reference-python-written streams decode to the reference's reconstruction",
                              "needs bit-identical h_s indexes; streams differ")


@gpu
def test_factorized_relu_vs_reference_golden(dev, golden_dir):
    """`bmshj2018-factorized-relu` (google.py:166-199) against the reference class (cnn_relu.npz, make_golden.py
    --stage cnn_relu)."""
    g = np.load(f"{golden_dir}/cnn_relu.npz")
    keys = json.load(open(f"{golden_dir}/state_keys.json"))["cnn"]["factorized_relu"]
    net = cnn.FactorizedPriorReLU(N, M)
    synth.load_synthetic(net, seed=11)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == keys
    net = net.to(dev)
    x = torch.from_numpy(np.load(f"{golden_dir}/cnn_zoo.npz")["x"]).to(dev)
    y = net.g_a(x[0])
    assert rel(y, g["y"]) <= 1e-5
    fw = net(x)
    assert rel(sub(fw["x_hat"], 5), g["xhat_fw"]) <= 1e-3
    bits = float((-torch.log2(fw["likelihoods"]["y"].double())).sum())
    assert abs(bits - g["bits_y"][0]) <= 2e-3 * g["bits_y"][0]
    gy = torch.Generator().manual_seed(5)
    y_hat = torch.round(3.0 * torch.randn((1,) + tuple(y.shape), generator=gy))[0].to(dev)
    assert rel(sub(net.g_s(y_hat), 5), g["xhat_synth"]) <= 1e-5
    out = net.compress(x)
    assert list(out["shape"]) == list(g["shape"])
    same = out["strings"][0][0] == g["string0"].tobytes()
    print("factorized-relu: stream identical to the reference python's:", same, len(out["strings"][0][0]), len(g["string0"]))
    assert abs(len(out["strings"][0][0]) - len(g["string0"])) <= 8
    rec = net.decompress(out["strings"], out["shape"])
    assert rel(sub(rec["x_hat"], 5), g["xhat_rt"]) <= (1e-5 if same else 1e-3)


def test_cnn_zoo_entry_errors():
    with pytest.raises(ValueError, match="architecture"):
        cnn.cnn_model("nope", 1)
    with pytest.raises(ValueError, match="quality"):
        cnn.cnn_model("bmshj2018-hyperprior", 9)
    with pytest.raises(RuntimeError, match="Pre-trained"):
        cnn.cnn_model("mbt2018-mean", 3, pretrained=True)
    m = cnn.cnn_model("bmshj2018-factorized", 6)
    assert (m.N, m.M) == (192, 320)
    from cra5_amd import zoo
    h = zoo.bmshj2018_hyperprior(2)
    assert isinstance(h, cnn.ScaleHyperprior) and (h.N, h.M) == (128, 192)
    with pytest.raises(ValueError, match="between"):
        zoo.mbt2018_mean(0)
    with pytest.raises(RuntimeError, match="not yet available"):
        zoo.bmshj2018_factorized(1, pretrained=True)
    r = zoo.bmshj2018_factorized_relu(7)
    assert isinstance(r, cnn.FactorizedPriorReLU) and (r.N, r.M) == (192, 320)


# ---- production widths against the float64 oracle (torch_ref.cnn_*) ------------------------------------------------
# bmshj2018-hyperprior quality 6 = (N, M) = (192, 320), mbt2018-mean quality 3 = (128, 192), synthetic weights (seed 11)
# on a 3 x 128 x 192 image, batch 2.  Stage by stage: each oracle stage gets the input the GPU stage received, so a
# round() flip in one stage cannot fail the next.  The synthetic weights are used as they are: the activation bands
# below (measured on the oracle, asserted first) show they are not degenerate at these widths.

WIDE = [("bmshj2018-hyperprior", 6, "hyperprior", (192, 320)), ("mbt2018-mean", 3, "meanscale", (128, 192))]


def _rms(t):
    return float(torch.sqrt(torch.mean(t.detach().double().cpu() ** 2)))


def _sd64(net):
    return {k: v.detach().double().cpu() for k, v in net.state_dict().items()}


def _wide_input():
    return torch.rand(2, 3, 128, 192, generator=torch.Generator().manual_seed(77))


def _wide_y_hat(M):
    return torch.round(3.0 * torch.randn(1, M, 8, 12, generator=torch.Generator().manual_seed(5)))[0]


def _check_stages(net, x, arch, ref_tag):
    """g_a, h_a, h_s, g_s of `net` (on the GPU) against the oracle in float64 on the GPU stages' own inputs."""
    from oracle import torch_ref as R
    sd = _sd64(net)
    dev = x.device
    y = net.g_a(x)
    e_y = rel(y, R.cnn_g_a(x[None].double().cpu(), sd, arch)[0])
    y64 = y.double().cpu()[None]
    z = net.h_a(net._h_a_in(y))
    e_z = rel(z, R.cnn_h_a(y64 if arch == "meanscale" else y64.abs(), sd, arch)[0])
    z_hat = net._eb(z, ("z_hat",))["z_hat"].reshape(z.shape)
    p = net.h_s(z_hat)
    e_p = rel(p, R.cnn_h_s(z_hat.double().cpu()[None], sd, arch)[0])
    y_hat = _wide_y_hat(net.M).to(dev)
    xs = net.g_s(y_hat)
    e_x = rel(xs, R.cnn_g_s(y_hat.double().cpu()[None], sd, arch)[0])
    print(f"{ref_tag}: g_a rel {e_y:.2e}, h_a rel {e_z:.2e}, h_s rel {e_p:.2e}, g_s rel {e_x:.2e}")
    assert max(e_y, e_z, e_p, e_x) <= 1e-5, (e_y, e_z, e_p, e_x)
    return y, z, p, xs


@gpu
@pytest.mark.parametrize("arch,q,tag,NM", WIDE)
def test_cnn_production_width_vs_oracle(dev, arch, q, tag, NM):
    from oracle import torch_ref as R
    net = cnn.cnn_model(arch, q)
    assert (net.N, net.M) == NM
    synth.load_synthetic(net, seed=11)
    net = net.to(dev)
    x = _wide_input().to(dev)
    # non-degenerate activations first (bands hold with a wide margin: y rms 0.87 / 0.98, z 1.25 / 0.95, h_s 0.09 /
    # 0.08 with half of it > 0, g_s(y_hat) 1.3e3 / 2.1e2 on the oracle)
    sd = _sd64(net)
    y64 = R.cnn_g_a(x[:1].double().cpu(), sd, tag)
    assert 0.3 < _rms(y64) < 3.0
    h = F.conv2d(y64 if tag == "meanscale" else y64.abs(), sd["h_a.0.weight"], sd["h_a.0.bias"], padding=1)
    assert 0.2 < float((h > 0).double().mean()) < 0.8                                # h_a's first activation
    z64 = R.cnn_h_a(y64 if tag == "meanscale" else y64.abs(), sd, tag)
    assert 0.3 < _rms(z64) < 3.0 and float((torch.round(z64) != 0).double().mean()) > 0.3
    p64 = R.cnn_h_s(torch.round(z64), sd, tag)
    assert 0.01 < _rms(p64) < 1.0 and 0.2 < float((p64 > 0).double().mean()) < 0.8
    assert 10.0 < _rms(R.cnn_g_s(_wide_y_hat(net.M).double()[None], sd, tag)) < 1e4
    for b in range(2):
        _check_stages(net, x[b], tag, f"{arch} q{q} image {b}")


@gpu
@pytest.mark.parametrize("arch,q,tag,NM", WIDE)
def test_cnn_production_width_codec_consistency(dev, arch, q, tag, NM):
    """decompress(compress(x)) == g_s of the compress side's y_hat exactly (same kernels); batch 2 == two batch-1 calls;
    after loading a second synthetic seed the stages follow the new weights (the split-weight cache of _Conv / _Deconv
    is keyed on the parameter's version, not only its address)."""
    net = cnn.cnn_model(arch, q)
    synth.load_synthetic(net, seed=11)
    net = net.to(dev)
    x = _wide_input().to(dev)
    out = net.compress(x)
    rec = net.decompress(out["strings"], out["shape"])["x_hat"]
    for b in range(2):
        y = net.g_a(x[b])
        y_hat = net._side(y, ("y_hat",))[2]["y_hat"].reshape(y.shape)
        assert torch.equal(rec[b], net.g_s(y_hat)), b
        one = net.compress(x[b:b + 1])
        assert [s[0] for s in one["strings"]] == [s[b] for s in out["strings"]] and one["shape"] == out["shape"]
    fw = net(x)
    for b in range(2):
        fb = net(x[b:b + 1])
        assert torch.equal(fw["x_hat"][b], fb["x_hat"][0])
        for k in fw["likelihoods"]:
            assert torch.equal(fw["likelihoods"][k][b], fb["likelihoods"][k][0])
    # stale weights: same parameter tensors (same data_ptr), new values
    ptr = net.g_a[0].weight.data_ptr()
    sd2 = synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=12)
    full = {k: v.clone() for k, v in net.state_dict().items()}
    full.update({k: v.to(dev) for k, v in sd2.items()})
    net.load_state_dict(full)
    assert net.g_a[0].weight.data_ptr() == ptr
    _check_stages(net, x[0], tag, f"{arch} q{q} seed 12 after load_state_dict")
