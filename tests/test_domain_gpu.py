"""Per-element error bounds of the arithmetic on every frame's path, on the device: the erfc-polynomial GELU of every
GEMM route, LayerNorm, the GaussianConditional likelihood, and the finiteness probe.  Inputs, float64 references and the
bounds B come from tests/domain_helpers.py; tests/test_domain_inputs_cpu.py shows each B sound (the fp32 restatement
within B / 2) and sensitive (every listed wrong variant outside it).  Here the kernels are held to the same B,
unchanged: |got - ref64| <= B on every element, plus the properties that hold bit for bit.  Every case prints one
`ERR ...` line with the measured max |err| / B ("Per-element error bounds", records them)."""
import numpy as np
import pytest
import torch

import domain_helpers as H
import exact_helpers as X
from cra5_amd import ops
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ GELU

_BLOCKS = {}


def _gelu_block(kind, a_base, b_base):
    """(x fp32, ref float64, B float64) numpy blocks [len(a_base), len(b_base)] for one engine's bound; computed once per
    (bound, operands) and shared"""
    key = (kind, a_base.tobytes(), b_base.tobytes())
    if key not in _BLOCKS:
        with np.errstate(all="ignore"):
            x = (a_base[:, None] + b_base[None, :]).astype(np.float32)           # fl32(a + b): the epilogue's accumulator
        ref = H.gelu_ref64(x)
        _BLOCKS[key] = (x, ref, (H.gelu_bound if kind == "poly" else H.gelu_f32_bound)(x, ref))
    return _BLOCKS[key]


def _gelu_launches(M, N, grid, f16_range):
    """(a [M], b [N], a_base, b_base, row index, column index) per launch of one grid"""
    if grid == "dense":
        a, b = H.gelu_dense_vectors(M, N)
        yield a, b, a[: min(M, 384)], b[: min(N, 256)], np.arange(M) % 384, np.arange(N) % 256
        return
    pts = H.gelu_point_list(f16_range=f16_range)
    ri = np.arange(M) % H.GELU_POINT_ROWS.size
    for off in range(0, pts.size, N):
        ci = (off + np.arange(N)) % pts.size
        yield H.GELU_POINT_ROWS[ri], pts[ci], H.GELU_POINT_ROWS, pts, ri, ci


def _gelu_route(dev, M, N, label, run, kind="poly", out="f32", grids=("dense", "points")):
    """run(a fp32 [M] device, bias fp32 [N] device) -> (the a the engine really read [M] fp32, output [M, N] fp32 values).
    out: 'f32' (an fp32 output), 'split' (hi + lo read back: the split store's own term is added to B), 'hi' (the f16
    hi plane alone: compared with the f16 rounding of ref -+ B)."""
    for grid in grids:
        worst, stats, n_launch = 0.0, None, 0
        for a, b, a_base, b_base, ri, ci in _gelu_launches(M, N, grid, f16_range=(out != "f32")):
            a_seen, got = run(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
            assert np.array_equal(a_seen.cpu().numpy(), a), f"{label}: the engine did not read the intended a"
            xb, refb, Bb = _gelu_block(kind, a_base, b_base)
            rid, cid = torch.from_numpy(ri).to(dev), torch.from_numpy(ci).to(dev)
            take = lambda blk: torch.from_numpy(blk).to(dev)[rid][:, cid]
            x, ref, B = take(xb), take(refb), take(Bb)
            fin = torch.isfinite(x)
            if out == "hi":
                lo_ok = got >= (ref - B).float().half().float()
                hi_ok = got <= (ref + B).float().half().float()
                bad = fin & ~(lo_ok & hi_ok)
                assert not bool(bad.any()), (f"{label} {grid}: {int(bad.sum())} f16 outputs outside f16(ref -+ B); first at "
                                             f"x = {float(x[bad][0])!r}: got {float(got[bad][0])!r}, ref {float(ref[bad][0])!r}")
                err = (got.double() - ref).abs() / (B + 2.0 ** -11 * ref.abs() + 2.0 ** -25)   # (reported; the interval is the check)
            else:
                if out == "split":
                    B = B + 2.0 ** -21 * ref.abs() + 2.0 ** -24
                err = (got.double() - ref).abs()
                err = torch.where(err == 0, torch.zeros_like(err), err / B)
            r = err[fin]
            rmax = float(r.max())
            if out != "hi" and not rmax <= 1.0:
                i = int(torch.nan_to_num(r, nan=float("inf")).argmax())
                raise AssertionError(f"{label} {grid}: |err| / B = {rmax:.3f} at x = {float(x[fin][i])!r}: got "
                                     f"{float(got[fin][i])!r}, ref {float(ref[fin][i])!r}, B {float(B[fin][i]):.3e}; "
                                     f"{int((~(r <= 1)).sum())} of {r.numel()} elements outside B")
            worst = max(worst, rmax)
            # what holds bit for bit
            xn, gn = x.cpu().numpy(), got.cpu().numpy()
            H.gelu_exact_expectations(xn, gn, f"{label} {grid}", saturates=False)
            big = (xn >= 9.0) & np.isfinite(xn)
            if out == "f32":
                want = xn[big]
            elif out == "split":
                want = sum(X.split_model(torch.from_numpy(xn[big]))).numpy()
            else:
                want = torch.from_numpy(xn[big]).half().float().numpy()
            assert np.array_equal(gn[big], want), f"{label} {grid}: x >= 9 must come out as x"
            if grid == "dense" and out != "hi":
                inside = fin & (x.abs() <= 9)
                e = (got.double() - ref)[inside]
                stats = (float(e.abs().max()), float(torch.sqrt(torch.mean(e * e))))
            n_launch += 1
        extra = f", over [-9, 9]: max |err| {stats[0]:.2e}, RMS {stats[1]:.2e}" if stats else ""
        print(f"ERR gelu {label} {M}x{N} {grid}: max |err| / B = {worst:.3f} in {n_launch} launch(es){extra}")


def _split_operands(M, N, a, dev, plane="both"):
    A = torch.zeros(M, 32, device=dev)
    A[:, 0] = a
    W = torch.zeros(N, 32, device=dev)
    W[:, 0] = 1.0
    sa, sw = ops.split_f16(A), ops.split_f16(W, "auto")
    pa, pw = sa.planes(), sw.planes()
    X.check_planes(A, pa[0], pa[1], 1.0, "A")                    # a is on the 22-bit grid: the split store is exact
    X.check_planes(W, pw[0], pw[1], sw.scale_inv, "W")
    assert sw.scale_inv == 2.0 ** -12                            # a power of two: acc * wscale_inv is exact
    a_seen = pa[0][:, 0] if plane == "hi" else (pa[0][:, 0].double() + pa[1][:, 0].double()).float()
    return sa, sw, a_seen


def test_gelu_generic_epilogue(dev):
    """cra5_gemm_nt_split, fp32 and split output together at 333 x 260: edge tiles, the generic epilogue body"""
    M, N = 333, 260

    def run(which):
        def go(a, b):
            sa, sw, a_seen = _split_operands(M, N, a, dev)
            out_s = ops.SplitMat.empty(M, N, dev, zero=True)
            out = ops.gemm_nt_split(sa, sw, bias=b, gelu=True, out_split=out_s)
            return a_seen, (out if which == "f32" else out_s.to_float())
        return go
    _gelu_route(dev, M, N, "split GEMM, generic body, fp32 output", run("f32"))
    _gelu_route(dev, M, N, "split GEMM, generic body, split output", run("split"), out="split")


@pytest.mark.parametrize("M,N,tile", [(256, 256, "64x64"), (2048, 2048, "256x256"), (4224, 1024, "192x256")])
def test_gelu_straight_line_epilogue(dev, M, N, tile):
    """EPI_KIND 2 (split output only, interior tiles) in its three instantiations; then the reduced-precision mode, whose
    output is the f16 hi plane alone"""
    def run(hi_only):
        def go(a, b):
            sa, sw, a_seen = _split_operands(M, N, a, dev, plane="hi" if hi_only else "both")
            out_s = ops.SplitMat.empty(M, N, dev, zero=True)
            ops.gemm_nt_split(sa, sw, bias=b, gelu=True, out_split=out_s, want_f32=False, hi_only=hi_only)
            return a_seen, (out_s.planes()[0] if hi_only else out_s.to_float())
        return go
    _gelu_route(dev, M, N, f"split GEMM, straight-line body, {tile} tiles", run(False), out="split")
    _gelu_route(dev, M, N, f"split GEMM, straight-line body, {tile} tiles, hi_only", run(True), out="hi")


@pytest.mark.parametrize("M,N", [(648, 360), (100, 77)])
def test_gelu_small_engine(dev, M, N):
    """cra5_small_gemm_nt_split (csrc/hyper.hip: its own copy of gelu_erf)"""
    def go(a, b):
        sa, sw, a_seen = _split_operands(M, N, a, dev)
        return a_seen, ops.small_gemm_nt_split(sa, sw, bias=b, gelu=True)
    _gelu_route(dev, M, N, "small engine", go)


def test_gelu_exact_f32_engine(dev):
    """cra5_gemm_nt_f32: libm erff, 0.5 x (1 + erff(x / sqrt 2)) - held to ITS bound (absolute in the negative tail)"""
    M, N = 333, 260

    def go(a, b):
        A = torch.zeros(M, 32, device=dev)
        A[:, 0] = a
        W = torch.zeros(N, 32, device=dev)
        W[:, 0] = 1.0
        return a, ops.gemm_nt(A, W, bias=b, gelu=True)
    _gelu_route(dev, M, N, "exact-f32 engine", go, kind="f32")


# ------------------------------------------------------------------------------------------------ LayerNorm


def _ln_check(out, B, y, names, label, rows=None):
    r = H.ratio((out.double().cpu() - y).abs().numpy(), B.numpy())
    r = np.where(np.isnan(r), np.inf, r)
    if rows is not None:
        r = r[rows]
        names = [names[i] for i in rows]
    per_row = r.max(1)
    i = int(per_row.argmax())
    assert per_row[i] <= 1.0, (f"{label}: |err| / B = {per_row[i]:.3f} in row {i} ({names[i]}), column {int(r[i].argmax())}; "
                               f"rows outside B: {[names[j] for j in np.nonzero(per_row > 1)[0]]}")
    return float(per_row[i]), names[i]


@pytest.mark.parametrize("D", H.LN_DIMS)
def test_layernorm_rows(dev, D):
    """every row class at both sides of every template boundary, from a contiguous x and from a row-strided view into a
    row-strided output"""
    x, ga, be, names = H.ln_inputs(D)
    B, y, mean, var, rstd = H.ln_bound(x, ga, be)
    gd, bd = ga.to(dev), be.to(dev)
    out = ops.layernorm(x.to(dev), gd, bd, 1e-6)
    worst, where = _ln_check(out, B, y, names, f"layernorm D={D}")
    assert torch.equal(out[6].cpu(), be), "an all-zero row must come out as beta, bit for bit"
    big_x = torch.full((15, D + 12), float("nan"), device=dev)
    big_o = torch.full((15, D + 8), float("nan"), device=dev)
    big_x[:, 4:4 + D] = x.to(dev)
    xv, ov = big_x[:, 4:4 + D], big_o[:, 4:4 + D]
    assert xv.stride(0) == D + 12 and ov.stride(0) == D + 8
    ops.layernorm(xv, gd, bd, 1e-6, out=ov)
    assert torch.equal(ov, out), "the strided launch must give the contiguous launch's bits"
    assert bool(torch.isnan(big_o[:, :4]).all()) and bool(torch.isnan(big_o[:, 4 + D:]).all()), "a write outside the view"
    print(f"ERR layernorm D={D} (V4={H.ln_v4(D)}): max |err| / B = {worst:.3f} ({where}); strided launch bit-identical")


@pytest.mark.parametrize("D", (360, 1028))
def test_layernorm_nonfinite_rows_do_not_leak(dev, D):
    """one wave per row: a NaN row and a +inf row come out wholly non-finite, their neighbours in the same 4-row block
    stay within B"""
    x, ga, be, names = H.ln_inputs(D)
    x = x[[0, 1, 2, 3, 8, 9, 13, 14, 0]].clone()                   # 9 rows: blocks (0 1 2 3) (4 5 6 7) (8)
    names = [f"row {i}" for i in range(9)]
    x[1, D // 2] = float("nan")
    x[6, D - 1] = float("inf")
    clean = [0, 2, 3, 4, 5, 7, 8]
    xc = x.clone()
    xc[1], xc[6] = 0.0, 0.0
    B, y, *_ = H.ln_bound(xc, ga, be)
    out = ops.layernorm(x.to(dev), ga.to(dev), be.to(dev), 1e-6)
    assert not bool(torch.isfinite(out[1]).any()) and not bool(torch.isfinite(out[6]).any())
    worst, where = _ln_check(out, B, y, names, f"layernorm D={D}, non-finite neighbours", rows=clean)
    print(f"ERR layernorm D={D} clean rows beside a NaN row and an inf row: max |err| / B = {worst:.3f} ({where})")


# ------------------------------------------------------------------------------------------------ GaussianConditional


def test_gaussian_conditional_likelihood(dev):
    table = R.get_scale_table()
    y, mu, s, q = H.gc_inputs(table.numpy())
    ref = H.gc_ref64(q, mu, s)
    to = lambda a: torch.from_numpy(a).to(dev)
    o = ops.gaussian_conditional(to(s), to(mu), table.to(dev), y=to(y), want=("sym", "y_hat", "lik"))
    assert np.array_equal(o["sym"].cpu().numpy(), q), "rintf(y - mu) must be the intended integer"
    assert np.array_equal(o["y_hat"].cpu().numpy(), ref["yh"]), "y_hat = fl(q + mu), bit for bit"
    lik = o["lik"].cpu().numpy()
    r = H.ratio(np.abs(lik.astype(np.float64) - ref["ref"]), ref["B"])
    r = np.where(np.isnan(r), np.inf, r)
    i = int(r.argmax())
    assert r[i] <= 1.0, (f"|err| / B = {r[i]:.3f} at q = {q[i]}, mu = {mu[i]!r}, scale = {s[i]!r}: got {lik[i]!r}, "
                         f"ref {ref['ref'][i]!r}; {int((r > 1).sum())} of {r.size} elements outside B")
    deep = ref["lik64"] < 1e-9 * (1 - 1e-3)
    assert np.all(lik[deep] == np.float32(1e-9)), "below the clamp the likelihood is float32(1e-9), bit for bit"
    small = (ref["lik64"] >= 1e-9) & (ref["lik64"] < 1e-6)
    rel = np.abs(lik.astype(np.float64) - ref["ref"])[small] / ref["ref"][small]
    print(f"ERR gaussian_conditional lik, {r.size} elements ({deep.mean():.0%} clamped): max |err| / B = {r[i]:.3f}; "
          f"max relative error where 1e-9 <= lik < 1e-6: {rel.max():.2e}")


# ------------------------------------------------------------------------------------------------ the probe


def _probe(x, out, stride=1):
    out.fill_(float("nan"))                                         # written, not accumulated
    return ops.probe_sums(x, out, stride).cpu()


@pytest.mark.parametrize("n", H.PROBE_SIZES)
def test_probe_finds_every_position(dev, n):
    from cra5_amd.vaeformer import VAEformer
    g = torch.Generator().manual_seed(n)
    host = torch.randn(n, generator=g)
    x = host.to(dev)
    out = torch.empty(ops.PROBE_PARTIALS, device=dev)
    p = _probe(x, out)
    assert bool(torch.isfinite(p).all()), "every block stores its partial, a block with no element included"
    assert VAEformer._finite(p)
    err = abs(float(p.double().sum()) - float(host.double().sum()))
    tol = n * H.U * float(host.double().abs().sum())
    assert err <= tol, (err, tol)
    used = min(ops.PROBE_PARTIALS, -(-n // 256))
    assert bool((p[used:] == 0).all()), "a block past the data sums nothing"
    for pos in H.probe_positions(n):
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = float(host[pos])
            x[pos] = bad
            p = _probe(x, out)
            x[pos] = keep
            nf = (~torch.isfinite(p)).nonzero().view(-1).tolist()
            assert nf == [H.probe_block_of(pos)], f"n = {n}: {bad} at {pos} gave non-finite partials {nf}"
            assert not VAEformer._finite(p)
    # +inf and -inf that meet in one block (neighbouring lanes; and, 65536 apart, in one thread's own sum)
    pairs = [(0, 1)] if n > 1 else []
    if n > 65536:
        pairs.append((0, 65536))
    for i, j in pairs:
        ki, kj = float(host[i]), float(host[j])
        x[i], x[j] = float("inf"), float("-inf")
        p = _probe(x, out)
        x[i], x[j] = ki, kj
        assert not VAEformer._finite(p) and not bool(torch.isfinite(p[H.probe_block_of(i)]))
    assert torch.equal(x.cpu(), host)
    print(f"ERR probe n={n}: |sum of partials - float64 sum| / (n u sum |x|) = {err / tol:.2e}; "
          f"{len(H.probe_positions(n))} positions x (NaN, +inf, -inf) each found in its own partial")


@pytest.mark.parametrize("stride", (2, 3, 7))
def test_probe_stride_samples_every_stride_th_element(dev, stride):
    n = 70001
    assert n % stride
    g = torch.Generator().manual_seed(stride)
    host = torch.randn(n, generator=g)
    x = host.to(dev)
    out = torch.empty(ops.PROBE_PARTIALS, device=dev)
    cnt = -(-n // stride)
    p = _probe(x, out, stride)
    assert bool(torch.isfinite(p).all())
    sampled = host[::stride].double()
    assert sampled.numel() == cnt
    err, tol = abs(float(p.double().sum()) - float(sampled.sum())), cnt * H.U * float(sampled.abs().sum())
    assert err <= tol, (err, tol)
    for i in (0, 1, 255, 256, cnt // 2, cnt - 1):                   # sampled: found, in the partial of sample i
        keep = float(host[i * stride])
        x[i * stride] = float("nan")
        p = _probe(x, out, stride)
        x[i * stride] = keep
        assert (~torch.isfinite(p)).nonzero().view(-1).tolist() == [H.probe_block_of(i)], (stride, i)
    unsampled = [1, (cnt - 1) * stride - 1] + ([n - 1] if (n - 1) % stride else [])
    for j in unsampled:                                             # not sampled: by contract not seen
        assert j % stride
        keep = float(host[j])
        x[j] = float("nan")
        p = _probe(x, out, stride)
        x[j] = keep
        assert bool(torch.isfinite(p).all()), (stride, j)
    print(f"ERR probe stride={stride} n={n}: |sum - float64 sum of the sampled| / (cnt u sum |x|) = {err / tol:.2e}")


def test_probe_rejects_a_wrong_output_slice(dev):
    x = torch.zeros(1000, device=dev)
    for out in (torch.empty(2 * ops.PROBE_PARTIALS, device=dev)[::2], torch.empty(ops.PROBE_PARTIALS - 1, device=dev),
                torch.empty(ops.PROBE_PARTIALS + 1, device=dev)):
        with pytest.raises(TypeError):
            ops.probe_sums(x, out)
