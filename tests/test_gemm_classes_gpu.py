"""One launch set per class of cra5_gemm_nt_split (tests/gemm_class_helpers.py enumerates them from the form rule), at
the class's smallest grid shape, on exact-grid operands with non-zero lo planes:

  1. value: the fp32 output bit for bit against the three-product model with the class's product count; the split
     output by the rules of tests/test_exact_gpu.py; GELU classes inside domain_helpers.gelu_bound of the float64 GELU of
     the exact pre-activation;
  2. reduced precision: every lo half of A and W overwritten with an f16 NaN changes no output bit;
  3. which halves of a prefilled C_split the launch writes;
  4. chained classes: the residual aliasing C.

And every refused class: Cra5Error(CRA5_ERR_ARG), nothing written."""
import numpy as np
import pytest
import torch

import domain_helpers as H
import exact_helpers as X
import gemm_class_helpers as G
import split_helpers as S
from cra5_amd import ops
from cra5_amd._lib import Cra5Error, check, lib
from test_exact_gpu import _check_split_output

pytestmark = pytest.mark.gpu

_SHAPES = {}      # (M, N, Kp) -> the operands of one representative shape and their expectations, built once
PAT16 = torch.tensor(G.PATTERN, dtype=torch.int16)


class _Shape:
    def __init__(self, M, N, Kp, dev):
        a, w, b, r = (t.to(dev) for t in G.operands(M, N, Kp))
        self.sa, self.sw = ops.split_f16(a), ops.split_f16(w, "auto")
        self.pa, self.pw = self.sa.planes(), self.sw.planes()
        X.check_planes(a, self.pa[0], self.pa[1], 1.0, "A")
        X.check_planes(w, self.pw[0], self.pw[1], self.sw.scale_inv, "W")
        assert self.sw.scale_inv == 1.0 / G.W_SCALE and self.sa.Kp == Kp
        assert float(self.pa[1].abs().max()) > 0 and float(self.pw[1].abs().max()) > 0     # non-zero lo planes
        self.b, self.r, self.dev = b, r, dev
        self._exp, self._gelu, self._ops = {}, {}, {}

    def expectation(self, hi, res):
        """(float64 expectation, granule, max sum |term| in granules) of bias (+ res), the pre-activation without res"""
        if (hi, res) not in self._exp:
            self._exp[(hi, res)] = X.three_product_expectation(self.pa, self.pw, self.sw.scale_inv, hi_only=hi, bias=self.b,
                                                               res=self.r if res else None)
        return self._exp[(hi, res)]

    def gelu(self, hi):
        """(x fp32 pre-activation, float64 GELU, bound B) on the device; the bound is domain_helpers.gelu_bound"""
        if hi not in self._gelu:
            x = self.expectation(hi, False)[0].float().cpu().numpy()           # (exact: an fp32 number, asserted there)
            ref = H.gelu_ref64(x)
            self._gelu[hi] = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(self.dev) for t in (x, ref, H.gelu_bound(x, ref)))
        return self._gelu[hi]

    def operand(self, which, plain, poisoned):
        """A or W as the class reads it.  Clean: split rows, or plain rows (A in the first half of a split-pitch buffer,
        as the model's workspaces hold it; W as a packed plain copy).  Poisoned: every half the reduced-precision mode
        must not read holds an f16 NaN - the lo plane of split rows, the unused second half of a split-pitch plain row."""
        key = (which, plain, poisoned)
        if key not in self._ops:
            s = self.sa if which == "A" else self.sw
            if not plain:
                out = s
                if poisoned:
                    out = ops.SplitMat(s.data.clone(), s.rows, s.K, s.Kp, s.scale_inv)
                    out.data.view(s.rows, s.Kp // 32, 2, 32)[:, :, 1] = G.PATTERN
            elif which == "W" and not poisoned:
                out = s.plain_copy()
            else:
                out = X.plain_rows_of(s)
                out.scale_inv = s.scale_inv
                if poisoned:
                    out.data[:, s.Kp:] = G.PATTERN
            self._ops[key] = out
        return self._ops[key]


def _shape(c, dev):
    key = (c.M, c.N, c.Kp)
    if key not in _SHAPES:
        if len(_SHAPES) >= 4:                      # (the parameters are sorted by shape: old ones are not needed again)
            _SHAPES.pop(next(iter(_SHAPES)))
        _SHAPES[key] = _Shape(c.M, c.N, c.Kp, dev)
    return _SHAPES[key]


def _padded_split(M, N, dev, extra=3):
    """a C_split of M rows inside a buffer of M + extra, every half prefilled with the f16 NaN pattern"""
    Kp = (N + 31) // 32 * 32
    buf = torch.full((M + extra, 2 * Kp), G.PATTERN, dtype=torch.int16, device=dev)
    return buf, ops.SplitMat(buf[:M], M, N, Kp)


def _launch(sh, c, poisoned=False, **over):
    """one launch of the class's call -> (fp32 output or None, the padded C_split buffer or None, its SplitMat or None)"""
    hi = G.is_hi(c)
    A_ = sh.operand("A", bool(c.mode & ops.GEMM_A_PLAIN), poisoned)
    W_ = sh.operand("W", bool(c.mode & ops.GEMM_W_PLAIN), poisoned)
    out = torch.full((c.M, c.N), float("nan"), device=sh.dev) if c.outputs != "split" else None
    buf, out_s = _padded_split(c.M, c.N, sh.dev) if c.outputs != "f32" else (None, None)
    kw = dict(bias=sh.b, res=None if c.gelu else sh.r, gelu=c.gelu, out=out, out_split=out_s, want_f32=out is not None,
              hi_only=hi, out_plain=bool(c.mode & ops.GEMM_OUT_PLAIN), wide_k=bool(c.mode & ops.GEMM_WIDE_K))
    kw.update(over)
    got = ops.gemm_nt_split(A_, W_, **kw)
    assert (got is None) == (out is None) and (got is None or got.data_ptr() == kw["out"].data_ptr())
    return kw["out"], buf, out_s


def _stored(out_s, hi):
    """the values a consumer of C_split reads: hi + lo, or in the reduced-precision mode the hi plane / the plain row"""
    return out_s.planes()[0] if hi else out_s.to_float()


def _check_values(sh, c, key, out, out_s):
    hi = G.is_hi(c)
    n = 0
    if not c.gelu:
        e, g, worst = sh.expectation(hi, True)
        if out is not None:
            X.assert_exact(out, e, g, f"{key}: fp32 output")
            n += out.numel()
        if out_s is not None:
            if hi:       # the hi plane / the plain row holds f16(exact result), bit for bit
                X.assert_exact(_stored(out_s, True), e.float().half().double(), g, f"{key}: f16 rows of the split output")
            else:
                _check_split_output(out_s, e, key)
            n += out_s.rows * out_s.K
        return worst, n
    x, ref, B = sh.gelu(hi)
    worst = sh.expectation(hi, False)[2]
    fin = torch.isfinite(ref)
    assert bool(fin.all())
    if out is not None:
        X.assert_exact(out, ref, 2.0 ** -12, f"{key}: fp32 output, GELU", tol=B)
        n += out.numel()
    if out_s is not None:
        got = _stored(out_s, hi)
        if hi:           # the f16 rounding of a value inside ref -+ B (tests/test_domain_gpu.py, out='hi')
            ok = (got >= (ref - B).float().half().float()) & (got <= (ref + B).float().half().float())
            assert bool(ok.all()), f"{key}: {int((~ok).sum())} f16 outputs outside f16(ref -+ B)"
        else:
            X.assert_exact(got, ref, 2.0 ** -12, f"{key}: split output, GELU", tol=B + 2.0 ** -21 * ref.abs() + 2.0 ** -24)
        n += out_s.rows * out_s.K
    return worst, n


def _check_halves_written(c, key, out, buf, out_s):
    """check 3: the launch was given a C_split whose every half held the pattern"""
    hi, o_plain, M = G.is_hi(c), bool(c.mode & ops.GEMM_OUT_PLAIN), c.M
    pat = PAT16.to(buf.device)
    assert bool((buf[M:] == pat).all()), f"{key}: rows >= M of the C_split buffer were written"
    rows = buf[:M]
    if not hi:
        assert not bool((rows == pat).any()), f"{key}: a half of rows < M (pad columns included) was not written"
    elif o_plain:
        assert bool((rows[:, out_s.Kp:] == pat).all()), f"{key}: halves past the plain row were written"
        assert not bool((rows[:, : out_s.Kp] == pat).any()), f"{key}: a half of the plain row (pad included) was not written"
    else:
        v = rows.view(M, out_s.Kp // 32, 2, 32)
        n_lo = int((v[:, :, 1] != pat).sum())
        assert n_lo == 0, f"{key}: {n_lo} lo halves of C_split were written in the reduced-precision mode"
        assert not bool((v[:, :, 0] == pat).any()), f"{key}: a hi half (pad columns included) was not written"
    if out is not None:
        # both outputs: the raw storage is split_ref of the call's own fp32 output, padding and untouched halves included
        # (the rule of tests/test_split_store_gpu.py, here on a buffer prefilled with the pattern instead of zeros)
        S.compare_planes(rows.cpu().numpy(), out.cpu().numpy(), out_s.K, out_s.Kp, plain=o_plain, lo_written=not hi,
                         fill=G.PATTERN, label=key)


_ACCEPTED = sorted(G.accepted(), key=lambda kc: (kc[1].M, kc[1].N, kc[1].Kp, kc[0]))


@pytest.mark.parametrize("key,c", _ACCEPTED, ids=[k.replace(" ", ",") for k, _ in _ACCEPTED])
def test_gemm_class(dev, key, c):
    assert G.class_key(c) == key
    sh = _shape(c, dev)
    hi = G.is_hi(c)
    failed = []          # every check runs; a failing class names all the checks it fails

    def check(name, fn):
        try:
            return fn()
        except AssertionError as e:
            failed.append(f"check {name}: {e}")

    out, buf, out_s = _launch(sh, c)
    worst = sh.expectation(hi, not c.gelu)[2]
    n = (0 if out is None else out.numel()) + (0 if out_s is None else out_s.rows * out_s.K)
    check("1 (value)", lambda: _check_values(sh, c, key, out, out_s))
    if hi:               # check 2: no lo half of A / W is read
        out_p, buf_p, out_sp = _launch(sh, c, poisoned=True)

        def unread():
            assert out is None or torch.equal(out_p, out), f"{key}: the fp32 output changes with the lo planes of A / W poisoned"
            assert out_s is None or torch.equal(out_sp.planes()[0], out_s.planes()[0]), \
                f"{key}: the hi plane of the split output changes with the lo planes of A / W poisoned"
        check("2 (lo planes not read)", unread)
        n *= 2
    if out_s is not None:
        check("3 (halves of C_split written)", lambda: _check_halves_written(c, key, out, buf, out_s))
    if "K=chained" in key:   # check 4: the residual aliases C
        e, g, _ = sh.expectation(hi, True)
        x = sh.r.clone()
        _launch(sh, c, out=x, res=x)
        check("4 (in-place residual)", lambda: X.assert_exact(x, e, g, f"{key}: in-place residual"))
        n += x.numel()
    print(f"{key}: {c.M}x{c.N}x{c.Kp}, max sum |term| {worst:.3g} granules, {n} elements compared"
          + (f", FAILS checks {[f.split(':')[0] for f in failed]}" if failed else ""))
    assert not failed, "\n".join(failed)


def test_refused_classes_raise_and_write_nothing(dev):
    """one call per refused class.  Words ops.gemm_nt_split cannot spell (plain rows or CRA5_GEMM_WIDE_K without
    CRA5_GEMM_HI_ONLY: its own precondition) go to the C entry through the same status check."""
    ref = G.refused()
    assert ref
    for key, c in ref:
        sh = _shape(c, dev)
        hi = G.is_hi(c)
        out = torch.full((c.M, c.N), float("nan"), device=dev) if c.outputs != "split" else None
        buf, out_s = _padded_split(c.M, c.N, dev) if c.outputs != "f32" else (None, None)
        A_ = sh.operand("A", bool(c.mode & ops.GEMM_A_PLAIN), False)
        W_ = sh.operand("W", bool(c.mode & ops.GEMM_W_PLAIN), False)
        o_plain = bool(c.mode & ops.GEMM_OUT_PLAIN)
        with pytest.raises(Cra5Error) as ei:
            if hi:
                ops.gemm_nt_split(A_, W_, bias=sh.b, res=None if c.gelu else sh.r, gelu=c.gelu, out=out, out_split=out_s,
                                  want_f32=out is not None, hi_only=True, out_plain=o_plain, wide_k=bool(c.mode & ops.GEMM_WIDE_K))
            else:
                flags = G.call_flags(c) | ops.EPI_BIAS | (0 if c.gelu else ops.EPI_RES)
                if out_s is not None:
                    out_s.plain = o_plain
                check(lib().cra5_gemm_nt_split(A_.data.data_ptr(), A_.pitch, W_.data.data_ptr(), W_.pitch,
                                               None if out is None else out.data_ptr(), c.N,
                                               None if out_s is None else out_s.data.data_ptr(), 0 if out_s is None else out_s.pitch,
                                               sh.b.data_ptr(), sh.r.data_ptr(), c.N, c.M, c.N, c.Kp, float(W_.scale_inv), flags,
                                               None), "cra5_gemm_nt_split")
        assert ei.value.status == ops.ERR_ARG and "cra5_gemm_nt_split" in str(ei.value), key
        torch.cuda.synchronize()
        assert out is None or bool(torch.isnan(out).all()), f"{key}: the fp32 output was written"
        assert buf is None or bool((buf == PAT16.to(dev)).all()), f"{key}: C_split was written"
        print(f"{key}: {c.M}x{c.N}x{c.Kp} mode {c.mode:#x} gelu {c.gelu} out {c.outputs}: CRA5_ERR_ARG, nothing written")
