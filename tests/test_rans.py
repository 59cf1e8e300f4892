"""Entropy coder: product C++ (through the C ABI) vs the oracle C restatement vs the
independent pure-Python restatement - bit-exact streams, round trips, adversarial cases
(escape symbols, every table, empty / 1-symbol inputs, corrupt streams)."""
import numpy as np
import pytest

import entropy_helpers as E
from cra5_amd import ops
from cra5_amd._lib import Cra5Error
from oracle import cbind, rans_py
from oracle import torch_ref as R


def _random_tables(rng, ncdf, L):
    cdf = np.zeros((ncdf, L + 2), np.int32)
    lens = np.zeros(ncdf, np.int32)
    offs = np.zeros(ncdf, np.int32)
    for c in range(ncdf):
        n = int(rng.integers(2, L + 1))
        p = rng.random(n).astype(np.float32) ** int(rng.integers(1, 6))
        p /= p.sum()
        q = cbind.pmf_to_cdf(p)
        cdf[c, : n + 1] = q
        lens[c] = n + 1
        offs[c] = -int(rng.integers(0, n))
    return cdf, lens, offs


@pytest.mark.parametrize("seed", range(12))
def test_three_implementations_agree(seed):
    rng = np.random.default_rng(seed)
    cdf, lens, offs = _random_tables(rng, int(rng.integers(1, 9)), int(rng.integers(3, 60)))
    n = int(rng.integers(0, 4000))
    idx = rng.integers(0, cdf.shape[0], size=n).astype(np.int32)
    sym = rng.integers(-80, 80, size=n).astype(np.int32)
    if seed % 3 == 0 and n:
        sym[:: 5] = rng.integers(-(1 << 20), 1 << 20, size=sym[::5].size)  # long escape payloads
    a = ops.rans_encode(sym, idx, cdf, lens, offs)
    b = cbind.rans_encode(sym, idx, cdf, lens, offs)
    c = rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
    assert a == b == c
    assert len(a) % 4 == 0 and len(a) >= 8
    assert np.array_equal(ops.rans_decode(a, idx, cdf, lens, offs), sym)
    assert np.array_equal(cbind.rans_decode(a, idx, cdf, lens, offs).numpy(), sym)
    assert rans_py.RansDecoder().decode_with_indexes(a, idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist()) == sym.tolist()


def test_empty_and_single_symbol():
    rng = np.random.default_rng(1)
    cdf, lens, offs = _random_tables(rng, 2, 10)
    e = np.zeros(0, np.int32)
    s = ops.rans_encode(e, e, cdf, lens, offs)
    assert s == cbind.rans_encode(e, e, cdf, lens, offs) and len(s) == 8  # just the flushed state
    assert ops.rans_decode(s, e, cdf, lens, offs).size == 0
    one = np.array([0], np.int32)
    s = ops.rans_encode(one, one, cdf, lens, offs)
    assert s == cbind.rans_encode(one, one, cdf, lens, offs)
    assert ops.rans_decode(s, one, cdf, lens, offs).tolist() == [0]


def test_full_gaussian_tables_all_indexes():
    """Every one of the 64 default GC tables, symbols at and beyond both tails."""
    cdf, ln, off = [t.numpy() for t in R.gc_tables(R.get_scale_table(), cbind.pmf_to_cdf)]
    rng = np.random.default_rng(3)
    idx = np.repeat(np.arange(64, dtype=np.int32), 200)
    sigma = R.get_scale_table().numpy()[idx]
    sym = np.rint(rng.standard_normal(idx.size) * sigma * 1.5).astype(np.int32)
    sym[::50] = (-off[idx[::50]] + 3)        # just past the upper tail -> escape
    sym[1::50] = (off[idx[1::50]] - 3)       # just past the lower tail -> escape
    sym[2::50] = -off[idx[2::50]]            # exactly the last regular bin / escape boundary
    a = ops.rans_encode(sym, idx, cdf, ln, off)
    assert a == cbind.rans_encode(sym, idx, cdf, ln, off)
    assert np.array_equal(ops.rans_decode(a, idx, cdf, ln, off), sym)


def test_batch_api_threads():
    import ctypes
    from cra5_amd._lib import lib
    rng = np.random.default_rng(5)
    cdf, lens, offs = _random_tables(rng, 4, 30)
    streams = []
    for i in range(6):
        n = int(rng.integers(100, 5000))
        streams.append((rng.integers(-40, 40, size=n).astype(np.int32), rng.integers(0, 4, size=n).astype(np.int32)))
    ns = len(streams)
    VP = ctypes.c_void_p
    sym = (VP * ns)(*[s.ctypes.data for s, _ in streams])
    idx = (VP * ns)(*[i.ctypes.data for _, i in streams])
    n = (ctypes.c_size_t * ns)(*[s.size for s, _ in streams])
    cd = (VP * ns)(*[cdf.ctypes.data] * ns)
    ncd = (ctypes.c_int * ns)(*[cdf.shape[0]] * ns)
    st = (ctypes.c_int * ns)(*[cdf.shape[1]] * ns)
    ln = (VP * ns)(*[lens.ctypes.data] * ns)
    of = (VP * ns)(*[offs.ctypes.data] * ns)
    out = (VP * ns)()
    olen = (ctypes.c_size_t * ns)()
    rc = (ctypes.c_int * ns)()
    assert lib().cra5_rans_encode_batch(ns, sym, idx, n, cd, ncd, st, ln, of, out, olen, rc, 4) == 0
    blobs = [ctypes.string_at(out[i], olen[i]) for i in range(ns)]
    for i, (s, ix) in enumerate(streams):
        assert blobs[i] == ops.rans_encode(s, ix, cdf, lens, offs)
    dec = [np.empty(s.size, np.int32) for s, _ in streams]
    enc = (VP * ns)(*[ctypes.cast(ctypes.c_char_p(b), VP).value for b in blobs])
    elen = (ctypes.c_size_t * ns)(*[len(b) for b in blobs])
    dout = (VP * ns)(*[d.ctypes.data for d in dec])
    assert lib().cra5_rans_decode_batch(ns, enc, elen, idx, n, cd, ncd, st, ln, of, dout, rc, 3) == 0
    for d, (s, _) in zip(dec, streams):
        assert np.array_equal(d, s)
    for i in range(ns):
        lib().cra5_free(out[i])


def test_errors_are_codes_not_ub():
    rng = np.random.default_rng(2)
    cdf, lens, offs = _random_tables(rng, 2, 10)
    sym = np.zeros(4, np.int32)
    with pytest.raises(Cra5Error):
        ops.rans_encode(sym, np.array([0, 1, 2, 0], np.int32), cdf, lens, offs)  # index out of range
    good_idx = np.zeros(4, np.int32)
    s = ops.rans_encode(sym, good_idx, cdf, lens, offs)
    with pytest.raises(Cra5Error):
        ops.rans_decode(s[:4], good_idx, cdf, lens, offs)  # truncated
    with pytest.raises(ValueError):
        ops.rans_encode(sym, good_idx[:3], cdf, lens, offs)
    # a malformed table with a zero-width bin (cdf[v+1] == cdf[v]) is an error code, not a SIGFPE,
    # in the one-shot and in the buffered encoder (the reference divides by zero here)
    bad = cdf.copy()
    v = int(-offs[0])          # the bin symbol 0 of row 0 lands in
    bad[0, v + 1] = bad[0, v]
    with pytest.raises(Cra5Error):
        ops.rans_encode(sym, good_idx, bad, lens, offs)
    from cra5_amd import ans
    e = ans.BufferedRansEncoder()
    with pytest.raises(Cra5Error):
        e.encode_with_indexes(sym.tolist(), good_idx.tolist(), bad.tolist(), lens.tolist(), offs.tolist())
    assert len(e.flush()) == 8   # nothing was buffered by the failed push


def test_decoder_bucket_tables_wide_and_narrow_rows():
    """The decoder's per-row bucket tables (csrc/host_entropy.cpp) against the oracle's linear scan:
    rows from 2 bins to 3000 bins, bins of frequency 1 (many bins per bucket), every symbol of every
    row hit at least once, decode into a caller-provided buffer."""
    rng = np.random.default_rng(5)
    rows = []
    for n in (2, 3, 17, 64, 500, 3000):
        p = np.full(n, 1e-9, np.float32)
        hot = rng.integers(0, n, size=max(1, n // 8))
        p[hot] = rng.random(hot.size).astype(np.float32) + 0.05
        rows.append(cbind.pmf_to_cdf(p / p.sum()))
    L = max(len(r) for r in rows)
    cdf = np.zeros((len(rows), L), np.int32)
    lens = np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        cdf[i, : len(r)] = r
        lens[i] = len(r)
    offs = np.zeros(len(rows), np.int32)
    idx, sym = [], []
    for i, r in enumerate(rows):
        k = len(r) - 2                      # max_value: symbols 0..k-1 are regular, >= k escape
        reg = np.arange(0, k)
        idx += [i] * (reg.size + 3)
        sym += reg.tolist() + [k, k + 5, -3]
    idx, sym = np.array(idx, np.int32), np.array(sym, np.int32)
    perm = rng.permutation(idx.size)
    idx, sym = idx[perm], sym[perm]
    a = ops.rans_encode(sym, idx, cdf, lens, offs)
    assert a == cbind.rans_encode(sym, idx, cdf, lens, offs)
    out = np.empty(idx.size, np.int32)
    assert ops.rans_decode(a, idx, cdf, lens, offs, out=out) is out
    assert np.array_equal(out, sym)
    assert np.array_equal(cbind.rans_decode(a, idx, cdf, lens, offs).numpy(), sym)
    with pytest.raises(ValueError):
        ops.rans_decode(a, idx, cdf, lens, offs, out=np.empty(idx.size - 1, np.int32))
    with pytest.raises(ValueError):
        ops.rans_decode(a, idx, cdf, lens, offs, out=np.empty(idx.size, np.int64))


def _np_resolve(sym, idx, cdf, lens, offs):
    """element-by-element restatement of the resolve step (rans_interface.cpp:121-150): the cross-check of the
    vectorised entropy_helpers.resolve_ref, which the device kernel is held to in tests/test_entropy_ints_gpu.py"""
    sr = np.zeros(sym.size, np.uint32)
    raw = np.zeros(sym.size, np.uint32)
    esc = np.zeros(sym.size, np.uint8)
    for i in range(sym.size):
        ci = int(idx[i])
        mx = int(lens[ci]) - 2
        v = int(sym[i]) - int(offs[ci])
        r = 0
        if v < 0:
            r, v = -2 * v - 1, mx
        elif v >= mx:
            r, v = 2 * (v - mx), mx
        start = int(cdf[ci, v]) & 0xFFFF
        rng_ = (int(cdf[ci, v + 1]) - int(cdf[ci, v])) & 0xFFFF
        sr[i] = start | (rng_ << 16)
        raw[i] = r
        if v == mx:
            nn = 0
            while nn < 8 and (r >> (4 * nn)) != 0:
                nn += 1
            esc[i] = nn + 1
    return sr, raw, esc


@pytest.mark.parametrize("seed", range(4))
def test_resolved_encoder_writes_the_same_stream(seed):
    """cra5_rans_encode_resolved (symbols resolved against the tables beforehand - on the GPU in the
    product) == cra5_rans_encode_with_indexes, byte for byte, incl. escapes with 0..8 payload nibbles."""
    rng = np.random.default_rng(100 + seed)
    cdf, lens, offs = _random_tables(rng, int(rng.integers(1, 9)), int(rng.integers(3, 60)))
    n = int(rng.integers(1, 3000))
    idx = rng.integers(0, cdf.shape[0], size=n).astype(np.int32)
    sym = rng.integers(-40, 40, size=n).astype(np.int32)
    sym[::7] = rng.integers(-(1 << 27), 1 << 27, size=sym[::7].size)
    sym[::11] = offs[idx[::11]] + lens[idx[::11]] - 2          # exactly max_value: escape with raw = 0
    a = ops.rans_encode(sym, idx, cdf, lens, offs)
    sr, raw, esc = E.resolve_ref(sym, idx, cdf, lens, offs)[:3]
    for got, want in zip((sr, raw, esc), _np_resolve(sym, idx, cdf, lens, offs)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert ops.rans_encode_resolved(sr, raw, esc) == a
    assert ops.rans_encode_resolved(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8)) == \
        ops.rans_encode(np.zeros(0, np.int32), np.zeros(0, np.int32), cdf, lens, offs)
    bad = esc.copy()
    bad[0] = 255
    with pytest.raises(Cra5Error):
        ops.rans_encode_resolved(sr, raw, bad)


def test_decoder_rejects_garbage_without_ub():
    """Random bytes / a non-monotone table decode to an error code or to symbols, never to a crash."""
    rng = np.random.default_rng(9)
    cdf, lens, offs = _random_tables(rng, 3, 20)
    idx = rng.integers(0, 3, size=500).astype(np.int32)
    for k in range(20):
        junk = rng.integers(0, 256, size=int(rng.integers(8, 400)), dtype=np.uint8).tobytes()
        try:
            ops.rans_decode(junk, idx, cdf, lens, offs)
        except Cra5Error:
            pass
    bad = cdf.copy()
    bad[0, 1], bad[0, 2] = bad[0, 2], bad[0, 1]      # not sorted: generic search path
    sym = np.zeros(50, np.int32)
    s = ops.rans_encode(sym, np.ones(50, np.int32), cdf, lens, offs)
    try:
        ops.rans_decode(s, np.zeros(50, np.int32), bad, lens, offs)
    except Cra5Error:
        pass


def test_product_pmf_to_cdf_matches_reference(golden_dir):
    import json
    g = json.load(open(f"{golden_dir}/pmf_cdf.json"))
    for c in g["cases"]:
        assert ops.pmf_to_quantized_cdf(np.array(c["pmf"], dtype=np.float32), c["precision"]).tolist() == c["cdf"]
    for e in g["errors"]:
        if e["raises"]:
            with pytest.raises(ValueError):  # std::domain_error -> ValueError in the reference binding
                ops.pmf_to_quantized_cdf(np.array([float(v) for v in e["pmf"]], dtype=np.float32))


def test_stateful_classes_match_reference_semantics():
    """cra5_amd.ans: BufferedRansEncoder (several pushes with DIFFERENT tables, one flush) and
    RansDecoder.set_stream/decode_stream, against the pure-Python oracle of the same classes."""
    from cra5_amd import ans
    rng = np.random.default_rng(11)
    ta = _random_tables(rng, 3, 20)
    tb = _random_tables(rng, 5, 40)
    groups = []
    for t in (ta, tb, ta):
        n = int(rng.integers(1, 800))
        groups.append((rng.integers(-60, 60, size=n).astype(np.int32),
                       rng.integers(0, t[0].shape[0], size=n).astype(np.int32), t))
    e, eo = ans.BufferedRansEncoder(), rans_py.BufferedRansEncoder()
    for sym, idx, (cdf, lens, offs) in groups:
        e.encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
        eo.encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
    stream = e.flush()
    assert stream == eo.flush()
    assert e.flush() == eo.flush()          # flushing an empty encoder: just the 8-byte state
    d, do = ans.RansDecoder(), rans_py.RansDecoder()
    d.set_stream(stream)
    do.set_stream(stream)
    for sym, idx, (cdf, lens, offs) in groups:
        got = d.decode_stream(idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
        assert got == sym.tolist() == do.decode_stream(idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
    # one-shot classes
    sym, idx, (cdf, lens, offs) = groups[1]
    s1 = ans.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
    assert s1 == rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist())
    assert ans.RansDecoder().decode_with_indexes(s1, idx.tolist(), cdf.tolist(), lens.tolist(), offs.tolist()) == sym.tolist()
    assert ans.pmf_to_quantized_cdf([0.25, 0.5, 0.25], 16) == [0, 16384, 49152, 65536]


def _kat_cases():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_rans_kat.py")
    spec = importlib.util.spec_from_file_location("make_rans_kat", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.cases()


def test_known_answer_inputs_roundtrip_and_agree():
    """The KAT inputs of tools/make_rans_kat.py (escape-heavy rows, both escape signs, 2^30
    payloads, 1- and 2-symbol streams): product == oracle C == oracle Python, and every decoder
    reads every stream back.  Runs everywhere; the byte-level pin needs rans_kat.npz (next test)."""
    for name, sym, idx, cdf, ln, off in _kat_cases():
        a = ops.rans_encode(sym, idx, cdf, ln, off)
        b = cbind.rans_encode(sym, idx, cdf, ln, off)
        assert a == b, name
        if sym.size <= 5000:
            c = rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), ln.tolist(),
                                                          off.tolist())
            assert a == c, name
        assert np.array_equal(ops.rans_decode(a, idx, cdf, ln, off), sym), name
        assert np.array_equal(cbind.rans_decode(a, idx, cdf, ln, off).numpy(), sym), name


def test_known_answer_streams_from_real_compressai(golden_dir):
    """Byte-level pin against a REAL compressai.ans build (rans_interface.cpp:108-284 + ryg_rans
    rans64.h).  tests/golden/rans_kat.npz is produced by tools/make_rans_kat.py on a machine where
    `import compressai` works; the build container has no such wheel and the reference cannot build
    its extension, so until the file is committed byte parity stays 'unpinned' (DESIGN section 2)."""
    import os
    path = os.path.join(golden_dir, "rans_kat.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/rans_kat.npz absent: run tools/make_rans_kat.py where compressai is installed")
    g = np.load(path)
    assert "SELFTEST" not in str(g["source"]), "rans_kat.npz was written by --selftest: not a known answer"
    for name, sym, idx, cdf, ln, off in _kat_cases():
        want = g[f"stream_{name}"].tobytes()
        assert ops.rans_encode(sym, idx, cdf, ln, off) == want, f"product encoder differs on {name}"
        assert cbind.rans_encode(sym, idx, cdf, ln, off) == want, f"oracle encoder differs on {name}"
        assert np.array_equal(ops.rans_decode(want, idx, cdf, ln, off), sym), f"product decoder differs on {name}"
        assert np.array_equal(cbind.rans_decode(want, idx, cdf, ln, off).numpy(), sym), name


def test_host_coder_under_address_and_ub_sanitizers():
    """The `asan` build flavour (cra5_amd/build.py; the reference's setup.py:72-75 has only a -O0 -g
    -UNDEBUG switch): the whole rANS suite above re-run in a subprocess against a host coder compiled
    with -fsanitize=address,undefined.  Any out-of-bounds read of a stream / table or signed overflow
    in the escape arithmetic aborts the subprocess."""
    import os
    import subprocess
    import sys
    from cra5_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = B.build(flavour="asan")
    rt = subprocess.check_output(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"],
                                 text=True).strip()
    if not os.path.exists(rt):
        pytest.skip("clang asan runtime not present")
    env = dict(os.environ, CRA5_LIB=lib, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_rans.py"), "-q", "-x",
                        "-k", "not sanitizers", "-p", "no:cacheprovider"], env=env, cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "passed" in r.stdout


@pytest.mark.parametrize("seed", range(4))
def test_compact_records_write_and_read_the_same_streams(seed):
    """Round 4: the frame path moves 16-bit escape records / uint8 indexes / int16 symbols between device and host coder
    (cra5_rans_encode_resolved_compact, cra5_rans_decode_with_indexes_u8_i16).  Same bytes as the 32-bit entry points on
    the same symbols; values that do not fit return CRA5_ERR_RANGE (the caller re-does that frame with 32-bit records)."""
    from cra5_amd._lib import ERR_RANGE
    rng = np.random.default_rng(100 + seed)
    cdf, lens, offs = _random_tables(rng, 64, 40)
    n = 20000
    idx = rng.integers(0, 64, n).astype(np.int32)
    sym = np.round(rng.standard_normal(n) * 30).astype(np.int32)      # plenty of escapes at both ends, |payload| < 4096
    ref = ops.rans_encode(sym, idx, cdf, lens, offs)
    # host restatement of the compact resolve (device kernel: tests/test_entropy_ints_gpu.py)
    sr, raw, _, rec, overflow = E.resolve_ref(sym, idx, cdf, lens, offs)
    assert raw.max() < 4096 and overflow == 0
    assert ops.rans_encode_resolved_compact(sr, rec) == ref
    out16 = np.empty(n, np.int16)
    ops.rans_decode_compact(ref, idx.astype(np.uint8), cdf, lens, offs, out16)
    assert np.array_equal(out16.astype(np.int32), sym)
    # a payload beyond 12 bits / a symbol beyond int16: CRA5_ERR_RANGE, never a wrong stream
    rec_bad = rec.copy()
    rec_bad[n // 2] = 0xFFFF
    with pytest.raises(Cra5Error) as ei:
        ops.rans_encode_resolved_compact(sr, rec_bad)
    assert ei.value.status == ERR_RANGE
    sym_big = sym.copy()
    sym_big[7] = 40000
    big_stream = ops.rans_encode(sym_big, idx, cdf, lens, offs)
    with pytest.raises(Cra5Error) as ei:
        ops.rans_decode_compact(big_stream, idx.astype(np.uint8), cdf, lens, offs, out16)
    assert ei.value.status == ERR_RANGE
    assert np.array_equal(ops.rans_decode(big_stream, idx, cdf, lens, offs), sym_big)     # the 32-bit route reads it


def test_compact_record_with_payload_bits_above_its_nibble_count_is_refused():
    """cra5_rans_encode_resolved_compact codes a record's payload as exactly its declared nibbles: a record with payload
    bits above them is malformed (the device resolver never writes one) and returns CRA5_ERR_INDEX instead of ORing the
    stray bits into the coder state."""
    sr = np.full(4, 4096 << 16, dtype=np.uint32)      # start 0, range 4096
    good = np.array([0, (1 + 1) << 12 | 0x5, (1 + 2) << 12 | 0x5A, (1 + 3) << 12 | 0xFFF], dtype=np.uint16)
    assert len(ops.rans_encode_resolved_compact(sr, good)) >= 8
    for bad in ((1 + 0) << 12 | 0x1, (1 + 1) << 12 | 0x10, (1 + 2) << 12 | 0x100):
        rec = good.copy()
        rec[2] = bad
        with pytest.raises(Cra5Error) as ei:
            ops.rans_encode_resolved_compact(sr, rec)
        assert ei.value.status == -2, hex(bad)      # CRA5_ERR_INDEX


# ---- round 6: a desynchronised stream is an error, not a picture -----------------------------------
# rans_interface.cpp:215-284 (the reference's decoder) hands back whatever symbols fall out of a stream decoded with
# indexes that are not the encoder's; the product's one-shot decoders check that the coder is back at RANS64_L with every
# word consumed (CRA5_ERR_DESYNC -> StreamDesyncError).


def _gaussian_like_case(rng, n):
    cdf, lens, offs = _random_tables(rng, 6, 40)
    idx = rng.integers(0, cdf.shape[0], size=n).astype(np.int32)
    sym = rng.integers(-30, 30, size=n).astype(np.int32)
    return cdf, lens, offs, idx, sym


@pytest.mark.parametrize("seed", range(8))
def test_one_flipped_index_is_refused(seed):
    from cra5_amd._lib import StreamDesyncError
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(200, 5000))
    cdf, lens, offs, idx, sym = _gaussian_like_case(rng, n)
    s = ops.rans_encode(sym, idx, cdf, lens, offs)
    assert np.array_equal(ops.rans_decode(s, idx, cdf, lens, offs), sym)
    n_desync = 0
    for k in rng.integers(0, n, size=12):
        bad = idx.copy()
        others = [r for r in range(cdf.shape[0]) if r != idx[k] and not np.array_equal(cdf[r], cdf[idx[k]])]
        bad[k] = others[int(rng.integers(0, len(others)))]
        # the desynchronised tail either runs into an impossible symbol / the end of the stream (CRA5_ERR_STREAM) or
        # decodes "successfully" into garbage - which the end-state check turns into CRA5_ERR_DESYNC.  Never symbols.
        with pytest.raises(Cra5Error) as ei:
            ops.rans_decode(s, bad, cdf, lens, offs)
        n_desync += isinstance(ei.value, StreamDesyncError)
        # the compact-record decoder (the frame path's) behaves the same
        with pytest.raises(Cra5Error):
            ops.rans_decode_compact(s, bad.astype(np.uint8), cdf, lens, offs, np.zeros(n, np.int16))
        # the oracle restates the REFERENCE: it returns symbols (wrong ones) or a stream error, it has no end-state check
    del n_desync   # (how often it is the END-STATE check that catches it: test_reference_decoder_semantics_are_silent_garbage)


def test_end_state_check_trailing_and_missing_words():
    from cra5_amd._lib import ERR_DESYNC, StreamDesyncError
    rng = np.random.default_rng(7)
    cdf, lens, offs, idx, sym = _gaussian_like_case(rng, 1000)
    s = ops.rans_encode(sym, idx, cdf, lens, offs)
    with pytest.raises(StreamDesyncError) as ei:
        ops.rans_decode(s + b"\0\0\0\0", idx, cdf, lens, offs)           # a word nobody coded
    assert ei.value.status == ERR_DESYNC
    with pytest.raises(StreamDesyncError):
        ops.rans_decode(s, idx[:-1], cdf, lens, offs)                    # one symbol short: state not back at RANS64_L
    with pytest.raises(Cra5Error):
        ops.rans_decode(s, np.concatenate([idx, idx[:1]]), cdf, lens, offs)   # one symbol too many
    # the empty stream is exactly the flushed initial state
    e = np.zeros(0, np.int32)
    assert ops.rans_decode(ops.rans_encode(e, e, cdf, lens, offs), e, cdf, lens, offs).size == 0
    with pytest.raises(StreamDesyncError):
        ops.rans_decode(s, e, cdf, lens, offs)                           # symbols left in the stream


def test_own_streams_never_trip_the_end_state_check():
    """Soak: 400 random streams (empty to 20 k symbols, escapes with 1-8 nibble payloads, every row width) through the
    one-shot, compact, resolved and batch routes - the check is silent on every stream this coder wrote."""
    rng = np.random.default_rng(11)
    for k in range(400):
        cdf, lens, offs = _random_tables(rng, int(rng.integers(1, 9)), int(rng.integers(3, 200)))
        n = int(rng.integers(0, 20000)) if k % 10 == 0 else int(rng.integers(0, 600))
        idx = rng.integers(0, cdf.shape[0], size=n).astype(np.int32)
        sym = rng.integers(-100, 100, size=n).astype(np.int32)
        if k % 4 == 0 and n:
            sym[::7] = rng.integers(-(1 << 27), 1 << 27, size=sym[::7].size)
        s = ops.rans_encode(sym, idx, cdf, lens, offs)
        assert np.array_equal(ops.rans_decode(s, idx, cdf, lens, offs), sym)
        if n and np.abs(sym).max() < 32768:
            out = np.zeros(n, np.int16)
            ops.rans_decode_compact(s, idx.astype(np.uint8), cdf, lens, offs, out)
            assert np.array_equal(out, sym)


def test_reference_decoder_semantics_are_silent_garbage():
    """What the check replaces.  On the codec's own Gaussian tables (escapes rare, every cumulative value lands in a real
    bin) the oracle - a restatement of rans_interface.cpp:215-284, which has no end-state check - decodes a stream with ONE
    neighbouring-row index (the cross-platform h_s flip of DESIGN.md section 2) into wrong symbols without complaint; the
    product refuses every such stream, and mostly it is the end-state check (CRA5_ERR_DESYNC) that does."""
    from cra5_amd._lib import StreamDesyncError
    cdf, ln, off = [t.numpy() for t in R.gc_tables(R.get_scale_table(), cbind.pmf_to_cdf)]
    table = R.get_scale_table().numpy()
    rng = np.random.default_rng(3)
    silent = caught_by_end_state = cases = 0
    for _ in range(20):
        n = 3000
        idx = rng.integers(0, 64, size=n).astype(np.int32)
        sym = np.rint(rng.standard_normal(n) * table[idx]).astype(np.int32)
        s = ops.rans_encode(sym, idx, cdf, ln, off)
        bad = idx.copy()
        k = int(rng.integers(0, n // 2))
        bad[k] = idx[k] + 1 if idx[k] < 63 else idx[k] - 1          # one step in the scale table
        cases += 1
        try:
            got = cbind.rans_decode(s, bad, cdf, ln, off).numpy()
            silent += int(not np.array_equal(got, sym))
        except Exception:  # noqa: BLE001 - the oracle refuses streams it would read past
            pass
        with pytest.raises(Cra5Error) as ei:
            ops.rans_decode(s, bad, cdf, ln, off)
        caught_by_end_state += isinstance(ei.value, StreamDesyncError)
    print(f"{cases} one-index flips: reference semantics silent garbage {silent}, product end-state check {caught_by_end_state}")
    assert silent >= cases // 2 and caught_by_end_state >= cases // 4     # (the others run out of words: CRA5_ERR_STREAM)


def test_encoder_reciprocal_division_is_exact_for_every_frequency():
    """Round 6: the encoder divides by a bin's frequency with a pre-computed reciprocal (mulhi + shift, the published
    rans64 Rans64EncPutSymbol form) instead of a 64-bit divide.  Every frequency 1 .. 65535 and its complement, as the two
    bins of a two-bin row, over states that wander through the coder's whole range: the product's stream equals the
    oracle's (plain `/` and `%`) byte for byte, through the one-shot encoder and through the resolved encoder; and it
    decodes."""
    rng = np.random.default_rng(21)
    freqs = np.arange(1, 65536, dtype=np.int32)
    cdf = np.zeros((freqs.size, 4), np.int32)
    cdf[:, 1] = freqs
    cdf[:, 2] = 65536
    lens = np.full(freqs.size, 3, np.int32)          # two bins: symbol 0 (freq f), symbol 1 = the escape bin (65536 - f)
    offs = np.zeros(freqs.size, np.int32)
    idx = np.repeat(np.arange(freqs.size, dtype=np.int32), 6)
    rng.shuffle(idx)
    sym = np.zeros(idx.size, np.int32)               # bin 0 only: no escape payloads, pure put() traffic ...
    a = ops.rans_encode(sym, idx, cdf, lens, offs)
    assert a == cbind.rans_encode(sym, idx, cdf, lens, offs)
    assert np.array_equal(ops.rans_decode(a, idx, cdf, lens, offs), sym)
    sym2 = rng.integers(0, 3, size=idx.size).astype(np.int32)      # ... and with the complement bin + escape payloads mixed in
    b = ops.rans_encode(sym2, idx, cdf, lens, offs)
    assert b == cbind.rans_encode(sym2, idx, cdf, lens, offs)
    assert np.array_equal(ops.rans_decode(b, idx, cdf, lens, offs), sym2)
    # three-bin rows: frequencies 1, f, 65535 - f, so that f = 1 and the largest frequencies meet mid-range states too
    cdf3 = np.zeros((freqs.size - 1, 5), np.int32)
    cdf3[:, 1] = 1
    cdf3[:, 2] = 1 + freqs[:-1]
    cdf3[:, 3] = 65536
    l3 = np.full(freqs.size - 1, 4, np.int32)
    o3 = np.zeros(freqs.size - 1, np.int32)
    i3 = rng.integers(0, freqs.size - 1, size=200000).astype(np.int32)
    s3 = rng.integers(0, 2, size=i3.size).astype(np.int32)
    c = ops.rans_encode(s3, i3, cdf3, l3, o3)
    assert c == cbind.rans_encode(s3, i3, cdf3, l3, o3)
    assert np.array_equal(ops.rans_decode(c, i3, cdf3, l3, o3), s3)
