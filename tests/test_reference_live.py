"""The PRODUCT's coder plugged in as the reference's `compressai.ans` (cra5_amd.ans, C ABI), called exactly as the
reference's entropy models call it (entropy_models.py:264-269 compress, :318-323 decompress: Python lists of symbols /
indexes, the quantized CDF table as a list of rows, lengths and offsets as lists), on the integers and tables the
reference's own Python produced for the thin frame (tests/golden/thin_e2e.npz, tables_default.npz): it must reproduce
the committed golden byte streams (written with the oracle coder) and round-trip to the reference's y_hat."""
import numpy as np

from cra5_amd import ans as product_ans


def _tables(t, kind):
    return (t[f"{kind}_cdf"].tolist(), t[f"{kind}_len"].reshape(-1).tolist(), t[f"{kind}_off"].reshape(-1).tolist())


def test_reference_python_with_product_coder(golden_dir):
    g = np.load(f"{golden_dir}/thin_e2e.npz")
    t = np.load(f"{golden_dir}/tables_default.npz")
    gc, eb = _tables(t, "gc"), _tables(t, "eb")
    # y: GaussianConditional.compress - symbols = round(y - means), indexes from the scales
    y_sym, y_idx = g["sym_full"].astype(np.int32).tolist(), g["idx_full"].astype(np.int32).tolist()
    y_string = product_ans.RansEncoder().encode_with_indexes(y_sym, y_idx, *gc)
    assert y_string == g["y_string"].tobytes(), "y stream differs"
    # z: EntropyBottleneck.compress - symbols = round(z - medians), index = channel
    z_sym = g["z_sym"]
    z_idx = np.broadcast_to(np.arange(z_sym.shape[1], dtype=np.int32).reshape(1, -1, 1, 1), z_sym.shape)
    z_string = product_ans.RansEncoder().encode_with_indexes(z_sym.reshape(-1).tolist(), z_idx.reshape(-1).tolist(), *eb)
    assert z_string == g["z_string"].tobytes(), "z stream differs"
    # decompress(return_format="latent"): values read back, y_hat = values + means
    assert product_ans.RansDecoder().decode_with_indexes(z_string, z_idx.reshape(-1).tolist(), *eb) == z_sym.reshape(-1).tolist()
    values = product_ans.RansDecoder().decode_with_indexes(y_string, y_idx, *gc)
    assert values == y_sym
    y_hat_sub = np.asarray(values, dtype=np.float32)[::37] + g["means_sub"]
    assert np.allclose(y_hat_sub, g["y_hat_sub"], atol=1e-6)
    print("REFERENCE+PRODUCT-CODER OK", len(y_string), len(z_string))
