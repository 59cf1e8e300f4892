"""Thin Python launchers over the C ABI.  torch tensors are containers only: every
function passes raw `data_ptr()`s + sizes + the current HIP stream to the native
library.  Device entry points refuse non-GPU tensors (no CPU fallback)."""
import contextlib
import ctypes
import functools
import os
import threading

import numpy as np
import torch

from ._lib import check, lib

EPI_BIAS, EPI_GELU, EPI_RES = 1, 2, 4                                                            # CRA5_EPI_*
GEMM_HI_ONLY, GEMM_A_PLAIN, GEMM_W_PLAIN, GEMM_OUT_PLAIN, GEMM_WIDE_K = 8, 16, 32, 64, 128       # CRA5_GEMM_*: the mode word
FORM_TILE, FORM_K64, FORM_CHAINED, FORM_PLAIN = 0x1c0, 1, 2, 4                                   # CRA5_FORM_*
ERR_ARG = -7                                                                                     # CRA5_ERR_ARG


_TLS = threading.local()


def _stream():
    s = getattr(_TLS, "stream", None)
    if s is not None:
        return s
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def stream_scope():
    """Inside the scope this thread's launches go to the stream that is torch's current one AT ENTRY, looked up once
    (torch.cuda.current_stream().cuda_stream costs 2.7 us per launch - 30 % of a launch's host time; a frame's GPU phase
    is ~150 launches on one stream).  Do not switch torch streams inside the scope."""
    prev = getattr(_TLS, "stream", None)
    _TLS.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        yield
    finally:
        _TLS.stream = prev


class ClockSampler:
    """Shader-clock telemetry (cra5_clock_probe): a host thread launches a one-wave probe of `window_us` every
    `period_ms` on its own stream while the workload runs; `summary()` gives the effective shader clock the probes saw.
    bench.py runs it over the timed region so that two JSON lines from two boxes can be told apart by the clock they
    sustained.  (Short probes, not a resident wave: a long kernel blocks the streams sharing its hardware queue.)"""

    def __init__(self, device, n_max=4096, period_ms=5.0, window_us=50):
        self.n_max, self.period, self.window = int(n_max), float(period_ms) * 1e-3, int(window_us * 100)
        self.buf = torch.zeros(4 * self.n_max, dtype=torch.int64, device=device)
        self.stream = torch.cuda.Stream(device=device)
        self.n, self._on, self._th = 0, False, None

    def probe(self):
        """one probe on the sampler's stream (callers that pace the probes themselves)"""
        if self.n >= self.n_max:
            return
        check(lib().cra5_clock_probe(ctypes.c_void_p(self.buf.data_ptr() + 32 * self.n), self.window,
                                     ctypes.c_void_p(self.stream.cuda_stream)), "cra5_clock_probe")
        self.n += 1

    def start(self):
        import time
        self.n, self._on = 0, True

        def run():
            while self._on and self.n < self.n_max:
                self.probe()
                time.sleep(self.period)
        self._th = threading.Thread(target=run, daemon=True, name="cra5-clock")
        self._th.start()

    def stop(self):
        self._on = False
        if self._th is not None:
            self._th.join()
            self._th = None
        self.stream.synchronize()

    def summary(self, w0=None, w1=None):
        """w0 / w1: keep the probes that lie inside this wall-clock window (cra5_clock_stamp values)."""
        import numpy as np
        if self.n < 1:
            return None
        b = self.buf.cpu().numpy()[: 4 * self.n].reshape(self.n, 4).astype(np.int64)
        ok = b[:, 2] > b[:, 0]
        if w0 is not None:
            ok &= (b[:, 0] >= w0) & (b[:, 2] <= w1)
        b = b[ok]
        if len(b) < 1:
            return None
        ghz = (b[:, 3] - b[:, 1]) / ((b[:, 2] - b[:, 0]) * 10.0)
        return {"shader_ghz_mean": float(ghz.mean()), "shader_ghz_p10": float(np.percentile(ghz, 10)),
                "shader_ghz_median": float(np.median(ghz)), "shader_ghz_p90": float(np.percentile(ghz, 90)),
                "probes": int(len(b)), "probe_window_us": self.window / 100.0,
                "span_ms": float((b[-1, 2] - b[0, 0]) / 1e5)}


class KernelTimer:
    """Per-launch device timing with HIP events recorded on the launch stream
    (cra5_event_* in the C ABI).  Used by bench.py for the `roofline` object: it brackets
    every launch of one kernel family, so sum(work) / sum(duration) is that kernel's
    achieved rate over the timed region."""

    def __init__(self, sample_every=1):
        """(thread-safe: frame threads record concurrently)
        sample_every = n: bracket every n-th launch only (per calling thread).  Event records
        are queue packets between the kernels; at ~400 timed launches per frame they cost ~5 %
        of the frame rate, sampling keeps the timed region honest."""
        self.records = {}   # kind -> list of (start_ev, stop_ev, work)
        self._free = []
        self._lock = threading.Lock()
        self.sample_every = max(1, int(sample_every))
        self._tls = threading.local()

    def _ev(self):
        with self._lock:
            if self._free:
                return self._free.pop()
        e = ctypes.c_void_p()
        check(lib().cra5_event_create(ctypes.byref(e)), "cra5_event_create")
        return e

    def start(self):
        if self.sample_every > 1:
            n = getattr(self._tls, "n", 0) + 1
            self._tls.n = n
            if n % self.sample_every:
                return None
        e = self._ev()
        check(lib().cra5_event_record(e, _stream()), "cra5_event_record")
        return e

    def stop(self, kind, start_ev, work):
        if start_ev is None:
            return
        e = self._ev()
        check(lib().cra5_event_record(e, _stream()), "cra5_event_record")
        with self._lock:
            self.records.setdefault(kind, []).append((start_ev, e, work))

    def summary(self):
        """kind -> dict(launches, work, ms). Synchronises on the recorded events."""
        out = {}
        with self._lock:
            records, self.records = self.records, {}
        for kind, recs in records.items():
            ms_tot, work, done = 0.0, 0.0, []
            for s, e, w in recs:
                ms = ctypes.c_float()
                check(lib().cra5_event_elapsed_ms(s, e, ctypes.byref(ms)), "cra5_event_elapsed_ms")
                ms_tot += ms.value
                work += w
                done += [s, e]
            with self._lock:       # frame threads pop from _free concurrently (_ev)
                self._free += done
            out[kind] = dict(launches=len(recs), work=work, ms=ms_tot)
        return out


TIMER = None  # set to a KernelTimer by bench.py
_UNTIMED = contextlib.nullcontext()


@contextlib.contextmanager
def _bracket(kind, work):
    ev = TIMER.start()
    yield
    TIMER.stop(kind() if callable(kind) else kind, ev, work)


def _timed(kind, work):
    """`with _timed(kind, work):` around a launch: TIMER's event bracket, booked as `kind` (a name, or a function giving
    it - called only when a timer runs) with `work` flops / bytes.  No timer: one shared no-op context."""
    return _UNTIMED if TIMER is None else _bracket(kind, work)


COPY_CHUNK = 32 << 20
COPY_THREADS = 8     # host threads of one staged copy; cra5_api / VAEformer pass RuntimeConfig.copy_threads explicitly


def copy_h2d_staged(dst, src_np, pinned, threads=None):
    """host numpy array (C-contiguous) -> device tensor `dst` of the same byte size, through the pinned tensor
    `pinned`, on the current stream (cra5_copy_h2d_staged): chunked, host memcpy overlapped with the DMA."""
    n = src_np.nbytes
    if not (src_np.flags["C_CONTIGUOUS"] and dst.is_cuda and dst.is_contiguous() and dst.numel() * dst.element_size() == n):
        raise ValueError("copy_h2d_staged: the host array must be C-contiguous and the device tensor contiguous, of the same byte size")
    if not (pinned.is_pinned() and pinned.numel() * pinned.element_size() >= n):
        raise ValueError("copy_h2d_staged: `pinned` must be a pinned tensor of at least the frame's byte size")
    check(lib().cra5_copy_h2d_staged(_p(dst), ctypes.c_void_p(src_np.ctypes.data), ctypes.c_void_p(pinned.data_ptr()),
                                     n, COPY_CHUNK, threads or COPY_THREADS, _stream()), "cra5_copy_h2d_staged")
    return dst


def copy_d2h_staged(dst_np, src, pinned, threads=None):
    """device tensor -> host numpy array through `pinned`; returns when `dst_np` holds the data."""
    n = dst_np.nbytes
    if not (dst_np.flags["C_CONTIGUOUS"] and dst_np.flags["WRITEABLE"] and src.is_cuda and src.is_contiguous()
            and src.numel() * src.element_size() == n):
        raise ValueError("copy_d2h_staged: the host array must be writeable and C-contiguous, the device tensor contiguous, "
                         "of the same byte size")
    if not (pinned.is_pinned() and pinned.numel() * pinned.element_size() >= n):
        raise ValueError("copy_d2h_staged: `pinned` must be a pinned tensor of at least the frame's byte size")
    check(lib().cra5_copy_d2h_staged(ctypes.c_void_p(dst_np.ctypes.data), _p(src), ctypes.c_void_p(pinned.data_ptr()),
                                     n, COPY_CHUNK, threads or COPY_THREADS, _stream()), "cra5_copy_d2h_staged")
    return dst_np


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("cra5_amd device op called with a non-GPU tensor: the HIP path is the only path "
                               "(the CPU restatement lives in oracle/ and is test infrastructure)")
        if t.dtype not in (torch.float32, torch.int32, torch.int16):
            raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    # (a plain int: every entry point declares its argtypes, ctypes converts int -> void * itself)
    return None if t is None else t.data_ptr()


def _row_stride(t):
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), "expected a 2-D tensor with unit inner stride"
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def gemm_nt(a, w, bias=None, res=None, gelu=False, out=None):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T).  a / w / res / out may be row-strided views."""
    _dev(a, w, bias, res, out)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_GELU if gelu else 0) | (EPI_RES if res is not None else 0)
    with _timed("gemm_nt_f32", 2.0 * M * N * K):
        check(lib().cra5_gemm_nt_f32(_p(a), _row_stride(a), _p(w), _row_stride(w), _p(out), _row_stride(out), _p(bias),
                                     _p(res), _row_stride(res) if res is not None else 0, M, N, K, flags, _stream()),
              "cra5_gemm_nt_f32")
    return out


class SplitMat:
    """A [rows, K] fp32 matrix in the split-f16 layout of csrc/gemm_split_f16.hip: `data` is a
    uint16 tensor [rows, 2*Kp] (128-byte chunks of 32 hi | 32 lo halves), Kp = K rounded up to
    32 (zero padded), value = (hi + lo) * scale_inv."""

    __slots__ = ("data", "rows", "K", "Kp", "scale_inv", "plain")

    def __init__(self, data, rows, K, Kp, scale_inv=1.0, plain=False):
        self.data, self.rows, self.K, self.Kp, self.scale_inv = data, rows, K, Kp, scale_inv
        # plain = True (reduced-precision mode, round 5): the rows hold PLAIN f16 - element n at half n, no lo plane; the
        # row pitch is data.shape[1] halves (2 * Kp when the plain row sits in the first half of a split-layout buffer, Kp
        # for a plain weight copy).  Set by the producer of each call.
        self.plain = plain

    @property
    def pitch(self):
        """what the C ABI takes as lda_kp / ldw_kp / ldc_split_kp: k-elements per split row, halves per plain row"""
        return self.data.shape[1] if self.plain else self.Kp

    def plain_copy(self):
        """A PLAIN f16 copy of this (weight) matrix: its hi plane, [rows, Kp] contiguous, same scale."""
        assert not self.plain
        hi = self.data.view(self.rows, self.Kp // 32, 2, 32)[:, :, 0].reshape(self.rows, self.Kp).contiguous()
        return SplitMat(hi, self.rows, self.K, self.Kp, self.scale_inv, plain=True)

    @staticmethod
    def empty(rows, K, device, zero=False):
        Kp = (K + 31) // 32 * 32
        # int16 storage (torch has no uint16 arithmetic; only the bytes matter)
        data = (torch.zeros if zero else torch.empty)((rows, 2 * Kp), device=device, dtype=torch.int16)
        return SplitMat(data, rows, K, Kp)

    def planes(self):
        """The stored halves as two fp32 [rows, K] tensors (hi, lo), NOT multiplied by scale_inv (tests: the operands the
        MFMAs really read).  A plain matrix has no lo plane: zeros."""
        if self.plain:
            hi = self.data.view(torch.float16)[:, : self.K].float()
            return hi, torch.zeros_like(hi)
        h = self.data.view(torch.float16).view(self.rows, self.Kp // 32, 2, 32).float()
        return (h[:, :, 0].reshape(self.rows, self.Kp)[:, : self.K].contiguous(),
                h[:, :, 1].reshape(self.rows, self.Kp)[:, : self.K].contiguous())

    def to_float(self):
        """Reconstruct the fp32 values (tests / debugging)."""
        if self.plain:
            return self.data.view(torch.float16)[:, : self.K].float() * self.scale_inv
        h = self.data.view(torch.float16).view(self.rows, self.Kp // 32, 2, 32).float()
        return ((h[:, :, 0] + h[:, :, 1]).reshape(self.rows, self.Kp)[:, : self.K]) * self.scale_inv


def split_f16(x, scale_pow2=None, out=None):
    """fp32 [rows, K] (row-strided ok) -> SplitMat.  scale_pow2: None = 1.0; 'auto' = the
    power of two that brings max|x| into [2^12, 2^13) (weights)."""
    _dev(x)
    rows, K = x.shape
    scale = 1.0
    if scale_pow2 == "auto":
        amax = float(x.abs().max())
        if amax > 0 and amax == amax and amax != float("inf"):
            import math
            scale = 2.0 ** (12 - math.floor(math.log2(amax)))
    elif scale_pow2 is not None:
        scale = float(scale_pow2)
    if out is None:
        out = SplitMat.empty(rows, K, x.device)
    check(lib().cra5_split_f16(_p(x), _row_stride(x), _p(out.data), rows, K, out.Kp, scale, _stream()),
          "cra5_split_f16")
    out.scale_inv = 1.0 / scale
    out.plain = False
    return out


@functools.lru_cache(maxsize=None)
def gemm_form(M, N, Kp, flags=0, f32_out=True, split_out=False):
    """cra5_gemm_split_form, memoised: the form cra5_gemm_nt_split gives a launch of this shape, these flags (EPI_* |
    GEMM_*) and these outputs - its tile's rows (& FORM_TILE) | FORM_K64 | FORM_CHAINED | FORM_PLAIN - or ERR_ARG where
    the launcher refuses.  THE rule lives in the library; nothing here or in the model restates it."""
    return lib().cra5_gemm_split_form(M, N, Kp, flags, f32_out, split_out)


@functools.lru_cache(maxsize=None)
def plain_ok(M, N, Kp):
    """Shapes on which cra5_gemm_nt_split takes plain-f16 operands / writes a plain output in the reduced-precision mode
    (the 64-wide k-step form by the launch's own size; Kp > 8192: the chained call, fp32 output alone - with a split
    output or a GELU the reduced-precision mode refuses Kp > 8192, plain rows or not)."""
    return gemm_form(M, N, Kp, GEMM_HI_ONLY | GEMM_A_PLAIN | GEMM_W_PLAIN | GEMM_OUT_PLAIN) >= 0


def _mode(hi_only, a=None, w=None, out_plain=False, wide_k=False):
    """The CRA5_GEMM_* mode word of a launch reading the SplitMats a / w: the reduced-precision mode, which operands are
    plain rows (their producers' tags), a plain split output, the forced 64-wide k-step form."""
    m = ((GEMM_A_PLAIN if a is not None and a.plain else 0) | (GEMM_W_PLAIN if w is not None and w.plain else 0)
         | (GEMM_OUT_PLAIN if out_plain else 0))
    assert hi_only or not m, "plain-f16 operands exist in the reduced-precision mode only"
    assert hi_only or not wide_k, "the 64-wide k-step form exists in the reduced-precision mode only"
    return m | (GEMM_HI_ONLY if hi_only else 0) | (GEMM_WIDE_K if wide_k else 0)


def _out_split(s, plain=False, gemm=False):
    """(pointer, pitch) of the optional split-f16 destination `s` (a SplitMat or None) for the C ABI, tagging its rows
    plain / split for its consumer.  The pitch is Kp; gemm: cra5_gemm_nt_split's, which counts a plain row in halves."""
    if s is None:
        return None, 0
    s.plain = bool(plain)
    return s.data.data_ptr(), s.pitch if gemm else s.Kp


def gemm_nt_split(a, w, bias=None, res=None, gelu=False, out=None, out_split=None, want_f32=True, hi_only=False,
                  out_plain=False, wide_k=False):
    """epi(a @ w^T) with a, w SplitMat (same K).  out: fp32 [M, N] (row-strided ok) unless
    want_f32=False; out_split: SplitMat [M, N] to receive the split-f16 result.  Reduced-precision mode (hi_only): a / w
    may be PLAIN matrices (SplitMat.plain) and out_plain=True writes out_split's rows plain; wide_k=True takes the
    64-wide k-step form (CRA5_GEMM_WIDE_K) at any size - the summation order of the big launches this one is a slice of.
    hi_only with K > 8192 exists as the chained call alone (no out_split, no gelu); otherwise Cra5Error(ERR_ARG)."""
    _dev(a.data, w.data, bias, res, out)
    M, N = a.rows, w.rows
    assert a.Kp == w.Kp and a.K == w.K, (a.K, w.K)
    assert a.scale_inv == 1.0, "activations are split unscaled"
    if out is None and want_f32:
        out = torch.empty((M, N), device=a.data.device, dtype=torch.float32)
    if out_split is not None:
        assert out_split.rows == M and out_split.K == N
    flags = ((EPI_BIAS if bias is not None else 0) | (EPI_GELU if gelu else 0) | (EPI_RES if res is not None else 0)
             | _mode(hi_only, a, w, out_plain, wide_k))
    cs, ldcs = _out_split(out_split, out_plain, gemm=True)

    def kind():   # booked by the kernel that runs: the 64 x 64-tile instantiation (hyper-prior and head GEMMs:
        # microseconds, launch-bound) apart from the big-tile kernels
        small = gemm_form(M, N, a.Kp, flags, out is not None, out_split is not None) & FORM_TILE == 64
        return "gemm_nt_split_small" if small else "gemm_nt_split"
    with _timed(kind, 2.0 * M * N * a.K):
        check(lib().cra5_gemm_nt_split(_p(a.data), a.pitch, _p(w.data), w.pitch, _p(out),
                                       _row_stride(out) if out is not None else 0, cs, ldcs, _p(bias), _p(res),
                                       _row_stride(res) if res is not None else 0, M, N, a.Kp, float(w.scale_inv),
                                       flags, _stream()), "cra5_gemm_nt_split")
    return out


def unembed_side_bytes(C, H, W, kh, kw, sh, sw):
    """Bytes of the side buffer of gemm_unembed for this geometry; 0: the fused form does not take it."""
    return int(lib().cra5_unembed_side_bytes(C, H, W, kh, kw, sh, sw))


def gemm_unembed(a, w, C, H, W, kh, kw, sh, sw, side, mean=None, std=None, out=None, hi_only=False):
    """Fused un-embed (cra5_gemm_nt_split_unembed): a SplitMat [Hp*Wp, K] (tokens), w SplitMat [C*kh*kw, K] -> the image
    x [C, H, W] (de-normalised when mean / std are given).  `side`: device float buffer of >= unembed_side_bytes()."""
    _dev(a.data, w.data, side, mean, std, out)
    assert a.Kp == w.Kp and a.K == w.K and w.rows == C * kh * kw and a.scale_inv == 1.0
    if out is None:
        out = torch.empty((C, H, W), device=a.data.device, dtype=torch.float32)
    assert out.is_contiguous() and tuple(out.shape) == (C, H, W) and side.is_contiguous()
    with _timed("gemm_nt_split", 2.0 * a.rows * w.rows * a.K):
        check(lib().cra5_gemm_nt_split_unembed(_p(a.data), a.pitch, _p(w.data), w.pitch, _p(out), _p(side),
                                               side.numel() * side.element_size(), _p(mean), _p(std), a.rows, a.Kp,
                                               float(w.scale_inv), C, H, W, kh, kw, sh, sw, _mode(hi_only, a, w), _stream()),
              "cra5_gemm_nt_split_unembed")
    return out


def small_gemm_nt_split(a, w, bias=None, res=None, gelu=False, out=None, out_split=None, want_f32=True,
                        unembed=None):
    """gemm_nt_split for the hyper-prior sizes (csrc/hyper.hip).  unembed = (Hz, Wz, p1, p2): `out` is the
    image [N / (p1*p2), Hz*p1, Wz*p2] and w's rows are in (c, p1, p2) order (HyperpriorDecoder un-embed)."""
    _dev(a.data, w.data, bias, res, out)
    M, N = a.rows, w.rows
    assert a.Kp == w.Kp and a.K == w.K, (a.K, w.K)
    assert a.scale_inv == 1.0, "activations are split unscaled"
    if unembed is not None:
        Hz, Wz, p1, p2 = unembed
        assert out is not None and out.is_contiguous() and out.numel() == M * N
    else:
        Hz = Wz = p1 = p2 = 0
        if out is None and want_f32:
            out = torch.empty((M, N), device=a.data.device, dtype=torch.float32)
    if out_split is not None:
        assert out_split.rows == M and out_split.K == N
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_GELU if gelu else 0) | (EPI_RES if res is not None else 0)
    cs, ldcs = _out_split(out_split)      # (split rows: workspace matrices change layout with the mode)
    with _timed("gemm_nt_split_small", 2.0 * M * N * a.K):
        check(lib().cra5_small_gemm_nt_split(_p(a.data), a.Kp, _p(w.data), w.Kp, _p(out),
                                             _row_stride(out) if (out is not None and unembed is None) else 0, cs, ldcs,
                                             _p(bias), _p(res), _row_stride(res) if res is not None else 0, M, N, a.Kp,
                                             float(w.scale_inv), flags, Hz, Wz, p1, p2, _stream()), "cra5_small_gemm_nt_split")
    return out


def hyper_attention(qkv, heads, out=None, out_split=None, want_f32=True):
    """Global attention of the hyper-prior blocks: qkv fp32 [n, 3C] -> [n, C] (exact fp32 MFMA)."""
    _dev(qkv, out)
    n, C3 = qkv.shape
    C = C3 // 3
    assert qkv.is_contiguous()
    if out is None and want_f32:
        out = torch.empty((n, C), device=qkv.device, dtype=torch.float32)
    if out_split is not None:
        assert out_split.rows == n and out_split.K == C
    os_, ldos = _out_split(out_split)
    with _timed("hyper_attention_f32", 4.0 * n * n * C):
        check(lib().cra5_hyper_attention_f32(_p(qkv), _p(out), os_, ldos, n, C, heads, float((C // heads) ** -0.5),
                                             _stream()), "cra5_hyper_attention_f32")
    return out if out is not None else out_split


def layernorm(x, gamma, beta, eps=1e-6, out=None, out_split=None, want_f32=True, out_plain=False):
    _dev(x, gamma, beta, out)
    rows, D = x.shape
    if out is None and want_f32:
        out = torch.empty((rows, D), device=x.device, dtype=torch.float32)
    if out_split is not None:
        assert out_split.rows == rows and out_split.K == D
    ys, ldys = _out_split(out_split, out_plain)
    # bytes: the row read once + every output written once
    # (the 648-row hyper-prior LayerNorms are launch-latency-bound: kept out of the HBM-bound figure)
    with _timed("layernorm" if rows >= 4096 else "layernorm_small",
                4.0 * rows * D * (1 + (out is not None) + (out_split is not None))):
        check(lib().cra5_layernorm_f32(_p(x), _row_stride(x), _p(gamma), _p(beta), _p(out),
                                       _row_stride(out) if out is not None else 0, ys, ldys, rows, D, float(eps),
                                       int(bool(out_plain)), _stream()), "cra5_layernorm_f32")
    return out if out is not None else out_split


def window_attention(qkv, pad_row, heads, H, W, wh, ww, out=None, out_split=None, want_f32=True):
    """qkv: [H*W, 3C] contiguous; returns [H*W, C] (fp32) and/or fills out_split (SplitMat,
    whose pad columns must already be zero)."""
    _dev(qkv, pad_row, out)
    N, C3 = qkv.shape
    C = C3 // 3
    assert N == H * W and qkv.is_contiguous() and pad_row.numel() == C3
    if out is None and want_f32:
        out = torch.empty((N, C), device=qkv.device, dtype=torch.float32)
    assert out is None or out.is_contiguous()
    if out_split is not None:
        assert out_split.rows == N and out_split.K == C
    scale = float((C // heads) ** -0.5)
    os_, ldos = _out_split(out_split)
    # algorithmic flops: real (unpadded) queries x all keys of their window, QK^T + PV
    with _timed("window_attention_f32", 4.0 * N * (wh * ww) * C):
        check(lib().cra5_window_attention_f32(_p(qkv), _p(pad_row), _p(out), os_, ldos, C, heads, H, W, wh, ww, scale,
                                              _stream()), "cra5_window_attention_f32")
    return out if out is not None else out_split


def attention_workspace_bytes(n_tokens, heads):
    """Bytes of device workspace the balanced whole-grid attention schedule wants for this shape (0: none)."""
    return int(lib().cra5_attention_workspace_bytes(int(n_tokens), int(heads)))


def attention_balanced_plan(n_tokens, heads):
    """(plan exists, workspace bytes it needs - possibly 0) of the balanced whole-grid attention schedule on this device."""
    nb = ctypes.c_size_t(0)
    ok = lib().cra5_attention_balanced_plan(int(n_tokens), int(heads), ctypes.byref(nb))
    return bool(ok), int(nb.value)


def window_attention_split(qkv_s, pad_s, heads, H, W, wh, ww, out=None, out_split=None, hi_only=False, workspace=None,
                           balanced=None):
    """qkv_s: SplitMat [H*W, 3C]; pad_s: SplitMat [1, 3C] (the split qkv bias).  workspace: a device byte tensor
    of >= attention_workspace_bytes(H*W, heads) -> the balanced schedule for whole-grid launches (balanced=True with
    workspace=None: a plan that needs no workspace)."""
    _dev(qkv_s.data, pad_s.data, out)
    N, C = qkv_s.rows, qkv_s.K // 3
    assert N == H * W and qkv_s.Kp == 3 * C and pad_s.Kp == 3 * C
    if out_split is not None:
        assert out_split.rows == N and out_split.K == C
    scale = float((C // heads) ** -0.5)
    # reduced-precision mode on PLAIN rows: the qkv GEMM wrote them plain; the pad row must be plain too and out_split is
    # written plain
    assert pad_s.plain == qkv_s.plain and (hi_only or not qkv_s.plain), \
        "plain qkv rows need the reduced-precision mode and a plain pad row"
    args = (_p(qkv_s.data), qkv_s.Kp, _p(pad_s.data), _p(out), *_out_split(out_split, qkv_s.plain), C, heads, H, W, wh, ww,
            scale, _mode(hi_only, qkv_s, out_plain=qkv_s.plain))
    with _timed("window_attention_split", 4.0 * N * (wh * ww) * C):
        if workspace is not None or balanced:
            assert workspace is None or (workspace.is_cuda and workspace.is_contiguous())
            check(lib().cra5_window_attention_split_ws(*args, _p(workspace),
                                                       workspace.numel() * workspace.element_size() if workspace is not None else 0,
                                                       _stream()), "cra5_window_attention_split_ws")
        else:
            check(lib().cra5_window_attention_split(*args, _stream()), "cra5_window_attention_split")
    return out if out is not None else out_split


MAX_WIN_TOKENS = 1152   # csrc/attention_split_f16.hip: windowed launches keep a per-block row-offset table


def split_attention_ok(C, heads, wh, ww, H=None, W=None):
    """Shapes the f16-MFMA attention kernel takes: head dim 64, window length a multiple of 32,
    and either the whole (H, W) grid as one window or a window of <= MAX_WIN_TOKENS tokens."""
    L = wh * ww
    return (C % heads == 0 and C // heads == 64 and L % 32 == 0
            and (L <= MAX_WIN_TOKENS or (wh == H and ww == W)))


def im2col(x, kh, kw, sh, sw, ldk=None, mean=None, std=None, out=None, out_split=None, out_plain=False):
    """x: [C,H,W] -> cols [Hp*Wp, ldk] (column (c*kh+i)*kw+j); pad columns are zero.  With
    out_split (a ZERO-initialised SplitMat [Hp*Wp, C*kh*kw]) the split-f16 form is written
    instead of the fp32 one."""
    _dev(x, mean, std, out)
    C, H, W = x.shape
    Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
    K = C * kh * kw
    assert x.is_contiguous()
    if out_split is not None:
        assert out_split.rows == Hp * Wp and out_split.K == K
        cs, ldk = _out_split(out_split, out_plain)
        with _timed("im2col", 4.0 * C * H * W + 4.0 * Hp * Wp * K):   # bytes: the frame read once + the patch matrix written once
            check(lib().cra5_im2col_f32(_p(x), _p(mean), _p(std), None, cs, C, H, W, kh, kw, sh, sw, Hp, Wp, ldk,
                                        int(bool(out_plain)), _stream()), "cra5_im2col_f32")
        return out_split
    ldk = ldk or K
    if out is None:
        out = torch.zeros((Hp * Wp, ldk), device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.shape[1] == ldk
    check(lib().cra5_im2col_f32(_p(x), _p(mean), _p(std), _p(out), None, C, H, W, kh, kw, sh, sw, Hp, Wp, ldk,
                                0, _stream()), "cra5_im2col_f32")
    return out


def col2im(cols, C, kh, kw, sh, sw, Hp, Wp, mean=None, std=None, out=None):
    _dev(cols, mean, std, out)
    H, W = (Hp - 1) * sh + kh, (Wp - 1) * sw + kw
    if out is None:
        out = torch.empty((C, H, W), device=cols.device, dtype=torch.float32)
    assert out.is_contiguous()
    with _timed("col2im", 4.0 * Hp * Wp * C * kh * kw + 4.0 * C * H * W):   # bytes: the column matrix read once + the frame written once
        check(lib().cra5_col2im_f32(_p(cols), _p(mean), _p(std), _p(out), C, H, W, kh, kw, sh, sw, Hp, Wp,
                                    _row_stride(cols), _stream()), "cra5_col2im_f32")
    return out


def gather_token_rows(src, out, Hp, Wp, ti0, n_ti, tj0, n_tj, ti_step=None, tj_step=None):
    """cra5_gather_token_rows: rows (ti0 + i) * Wp + (tj0 + j) mod Wp (i < n_ti, j < n_tj) of the token-major matrix `src`
    (Hp * Wp rows) -> rows i * n_tj + j of `out`, verbatim.  src / out: both SplitMat (split or plain rows; `out` takes
    src's layout) or both 2-D fp32 device tensors with unit inner stride.
    ti_step / tj_step (both given): cra5_gather_token_lattice - rows (ti0 + i * ti_step) * Wp + (tj0 + j * tj_step) mod Wp,
    the strided lattice of one token class of a thinned decode (subset.stride_plan)."""
    if isinstance(src, SplitMat):
        if not isinstance(out, SplitMat) or out.Kp != src.Kp or out.K != src.K or out.rows != n_ti * n_tj:
            raise ValueError("gather_token_rows: `out` must be a SplitMat of n_ti * n_tj rows and src's K")
        _dev(src.data, out.data)
        row_bytes = 2 * src.Kp if src.plain else 4 * src.Kp       # a plain row holds Kp halves, a split row 2 * Kp
        s_t, d_t = src.data, out.data
        out.scale_inv, out.plain = src.scale_inv, src.plain
    else:
        _dev(src, out)
        if out.dim() != 2 or src.dim() != 2 or out.shape[1] != src.shape[1] or out.shape[0] != n_ti * n_tj \
                or src.dtype != out.dtype:
            raise ValueError("gather_token_rows: `out` must be [n_ti * n_tj, K] of src's K and dtype")
        row_bytes = src.shape[1] * src.element_size()
        s_t, d_t = src, out
    if s_t.shape[0] != Hp * Wp:
        raise ValueError(f"gather_token_rows: src has {s_t.shape[0]} rows, the grid {Hp} x {Wp} tokens")
    es = s_t.element_size()
    if (ti_step is None) != (tj_step is None):
        raise ValueError("gather_token_rows: ti_step and tj_step come together")
    if ti_step is not None:
        check(lib().cra5_gather_token_lattice(_p(s_t), _row_stride(s_t) * es, _p(d_t), _row_stride(d_t) * es, row_bytes,
                                              Hp, Wp, ti0, ti_step, n_ti, tj0, tj_step, n_tj, _stream()),
              "cra5_gather_token_lattice")
        return out
    check(lib().cra5_gather_token_rows(_p(s_t), _row_stride(s_t) * es, _p(d_t), _row_stride(d_t) * es, row_bytes, Hp, Wp,
                                       ti0, n_ti, tj0, n_tj, _stream()), "cra5_gather_token_rows")
    return out


def strided_scatter(g, rows, cols, cls, n_cc, C, mean=None, std=None, out=None):
    """cra5_strided_scatter_f32: the thinned image [C, Ho, Wo] from the class matrices in the flat fp32 workspace `g`;
    rows int32 [Ho, 6], cols int32 [Wo, 3], cls int64 [n_rc * n_cc, 5]: device copies of subset.scatter_tables.  A seam
    row's point is its upper + lower partner, in that order; mean / std [C]: de-normalised (x * std[c] + mean[c])."""
    _dev(g, mean, std, out)
    ok = (g.is_contiguous() and g.dim() == 1 and all(t.is_cuda and t.is_contiguous() for t in (rows, cols, cls))
          and rows.dtype == torch.int32 and cols.dtype == torch.int32 and cls.dtype == torch.int64
          and rows.dim() == 2 and rows.shape[1] == 6 and cols.dim() == 2 and cols.shape[1] == 3
          and cls.dim() == 2 and cls.shape[1] == 5 and n_cc > 0 and cls.shape[0] % n_cc == 0)
    if not ok:
        raise ValueError("strided_scatter: g is a flat fp32 workspace; rows [Ho, 6] / cols [Wo, 3] int32 and cls "
                         "[n_rc * n_cc, 5] int64 contiguous device tables (subset.scatter_tables)")
    Ho, Wo = rows.shape[0], cols.shape[0]
    if out is None:
        out = torch.empty((C, Ho, Wo), device=g.device, dtype=torch.float32)
    if not (out.is_contiguous() and tuple(out.shape) == (C, Ho, Wo)):
        raise ValueError(f"strided_scatter: out must be a contiguous [{C}, {Ho}, {Wo}] tensor")
    with _timed("strided_scatter", 8.0 * C * Ho * Wo):
        check(lib().cra5_strided_scatter_f32(_p(g), g.numel(), _p(rows), _p(cols), _p(cls), cls.shape[0] // n_cc, n_cc,
                                             _p(mean), _p(std), _p(out), C, Ho, Wo, _stream()), "cra5_strided_scatter_f32")
    return out


def gather_token_list(src, out, tok):
    """cra5_gather_token_list: rows tok[r] of the token-major matrix `src` -> rows r of `out`, verbatim.  src / out: both
    SplitMat (split or plain rows; `out` takes src's layout) or both 2-D fp32 device tensors with unit inner stride; tok:
    a contiguous int32 device vector.  A tok[r] outside src's rows reads nothing: row r is all 0xFF bytes (NaN)."""
    if not (isinstance(tok, torch.Tensor) and tok.is_cuda and tok.dtype == torch.int32 and tok.dim() == 1
            and tok.is_contiguous() and tok.numel() > 0):
        raise ValueError("gather_token_list: tok must be a contiguous non-empty int32 device vector")
    n = tok.numel()
    if isinstance(src, SplitMat):
        if not isinstance(out, SplitMat) or out.Kp != src.Kp or out.K != src.K or out.rows != n:
            raise ValueError("gather_token_list: `out` must be a SplitMat of len(tok) rows and src's K")
        _dev(src.data, out.data)
        row_bytes = 2 * src.Kp if src.plain else 4 * src.Kp       # a plain row holds Kp halves, a split row 2 * Kp
        s_t, d_t, n_src = src.data, out.data, src.rows
        out.scale_inv, out.plain = src.scale_inv, src.plain
    else:
        _dev(src, out)
        if out.dim() != 2 or src.dim() != 2 or out.shape[1] != src.shape[1] or out.shape[0] != n or src.dtype != out.dtype:
            raise ValueError("gather_token_list: `out` must be [len(tok), K] of src's K and dtype")
        row_bytes = src.shape[1] * src.element_size()
        s_t, d_t, n_src = src, out, src.shape[0]
    if s_t.device != tok.device or d_t.device != tok.device or s_t.shape[0] < n_src:
        raise ValueError("gather_token_list: src, out and tok must lie on one device")
    es = s_t.element_size()
    check(lib().cra5_gather_token_list(_p(s_t), _row_stride(s_t) * es, _p(d_t), _row_stride(d_t) * es, row_bytes, n_src,
                                       _p(tok), n, _stream()), "cra5_gather_token_list")
    return out


_POINT_TABLES = (("rows", torch.int32), ("cols", torch.int32), ("rw", torch.float64), ("cw", torch.float64))
_POINT_PLAN_TABLES = _POINT_TABLES + (("pnode", torch.int32), ("tokens", torch.int32), ("contrib", torch.int32))


def points_tables(plan, device):
    """The device tables of ops.points_from_image (points.Points.taps: rows / cols int32 [P, 2], rw / cw fp64 [P, 2]) and,
    for a Points.plan, of ops.gather_token_list / ops.points_from_cols as well (pnode int32 [P, 4], tokens int32 [M],
    contrib int32 [n_nodes, 4]): the plan's geometry plus those copies."""
    return _device_tables(plan, plan, _POINT_PLAN_TABLES if "contrib" in plan else _POINT_TABLES, device)


def _points_args(what, t, spec, src, out, C):
    _dev(src, out)
    ok = isinstance(t, dict) and all(isinstance(t.get(k), torch.Tensor) and t[k].is_cuda and t[k].is_contiguous()
                                     and t[k].dtype == dt and t[k].device == src.device for k, dt in spec)
    if not ok:
        raise ValueError(f"{what}: tables must come from ops.points_tables (contiguous int32 / fp64 tensors on the source's "
                         "device)")
    P = int(t["P"])
    shapes = dict(rows=(P, 2), cols=(P, 2), rw=(P, 2), cw=(P, 2), pnode=(P, 4))
    if any(k in shapes and tuple(t[k].shape) != shapes[k] for k, _ in spec):
        raise ValueError(f"{what}: the tables do not belong to a plan of {P} points")
    if out is None:
        out = torch.empty((C, P), device=src.device, dtype=torch.float32)
    if not (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == C * P and out.shape[0] == C
            and out.shape[-1] == P and out.device == src.device):
        raise ValueError(f"{what}: out must be a contiguous fp32 [{C}, {P}] tensor on the source's device")
    return P, out


def points_from_cols(cols, tables, C, mean=None, std=None, out=None):
    """cra5_points_from_cols: the plan's P points out of the column matrix cols (fp32 [M, >= C * kh * kw], unit inner
    stride: the two-call un-embed of the plan's tokens, in their order, for C channels) -> fp32 [C, P].  tables:
    points_tables(Points.plan(...), device).  mean / std [C]: de-normalised per node (x * std[c] + mean[c]) before the
    interpolation."""
    _dev(mean, std)
    spec = tuple(s for s in _POINT_PLAN_TABLES if s[0] not in ("rows", "cols", "tokens"))
    P, out = _points_args("points_from_cols", tables, spec, cols, out, C)
    t = tables
    kh, kw = t["patch"][:2]
    M = int(t["tokens"].numel()) if isinstance(t.get("tokens"), torch.Tensor) else -1
    if cols.dtype != torch.float32 or cols.dim() != 2 or cols.shape[0] != M or cols.shape[1] < C * kh * kw \
            or t["contrib"].dim() != 2 or t["contrib"].shape[1] != 4:
        raise ValueError(f"points_from_cols: cols must be fp32 [{M} tokens, >= {C * kh * kw}] - the plan's token list x the "
                         f"channels' {kh * kw} products (got {tuple(cols.shape)} {cols.dtype})")
    with _timed("points_from_cols", 4.0 * C * P * 5):
        check(lib().cra5_points_from_cols(_p(cols), _row_stride(cols), M, C, kh * kw, _p(t["contrib"]), t["contrib"].shape[0],
                                          _p(t["pnode"]), _p(t["rw"]), _p(t["cw"]), P, int(t["method"] == "nearest"),
                                          _p(mean), _p(std), _p(out), _stream()), "cra5_points_from_cols")
    return out


def points_from_image(x, tables, out=None):
    """cra5_points_from_image: the contiguous fp32 device image x [C, H, W] at the plan's P points -> fp32 [C, P].  tables:
    points_tables(Points.taps(H, W) | Points.plan(H, W, ...), device) - the grid (H, W) is the plan's."""
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("points_from_image: x must be a contiguous fp32 [C, H, W] device tensor")
    C, H, W = x.shape
    P, out = _points_args("points_from_image", tables, _POINT_TABLES, x, out, C)
    t = tables
    if tuple(t["grid"]) != (H, W):
        raise ValueError(f"points_from_image: the tables were built for a {tuple(t['grid'])} grid, x is {(H, W)}")
    with _timed("points_from_image", 4.0 * C * P * 5):
        check(lib().cra5_points_from_image(_p(x), C, H, W, _p(t["rows"]), _p(t["cols"]), _p(t["rw"]), _p(t["cw"]), P,
                                           int(t["method"] == "nearest"), _p(out), _stream()), "cra5_points_from_image")
    return out


def crop(src, r0, Hb, c0, Wb, out=None):
    """cra5_crop_f32: out[c][i][j] = src[c][r0 + i][(c0 + j) mod Ws] - the box [C, Hb, Wb] of the contiguous image
    src [C, Hs, Ws], columns wrapping at its east edge."""
    _dev(src, out)
    C, Hs, Ws = src.shape
    if out is None:
        out = torch.empty((C, Hb, Wb), device=src.device, dtype=torch.float32)
    if not (src.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (C, Hb, Wb)):
        raise ValueError(f"crop: src must be contiguous and out a contiguous [{C}, {Hb}, {Wb}] tensor")
    with _timed("crop", 8.0 * C * Hb * Wb):
        check(lib().cra5_crop_f32(_p(src), C, Hs, Ws, _p(out), r0, Hb, c0, Wb, _stream()), "cra5_crop_f32")
    return out


_COARSEN_TABLES = (("row0", torch.int32), ("ntap", torch.int32), ("rw", torch.float64))
_REGRID_TABLES = _COARSEN_TABLES + (("order", torch.int32), ("col0", torch.int32), ("ctap", torch.int32),
                                    ("cw", torch.float64), ("tiles", torch.int32))
# per operator: its device tables, where they come from, what their plan counts (the words of two messages)
_WINDOW_OPS = {
    "coarsen": (_COARSEN_TABLES, "plan_tables must come from ops.coarsen_tables (row0 / ntap int32, rw fp64 contiguous "
                "device tensors)", "{Ho} output rows"),
    "regrid": (_REGRID_TABLES, "tables must come from ops.regrid_tables (row0 / ntap / order / col0 / ctap / tiles int32, "
               "rw / cw fp64 contiguous device tensors)", "{Ho} x {Wo} target points"),
}


def _device_tables(plan, host, spec, device):
    """dict(plan) with device copies of the host arrays host[name] for every (name, dtype) of spec."""
    t = dict(plan)
    for k, dt in spec:
        t[k] = torch.as_tensor(np.ascontiguousarray(host[k], dtype=np.float64 if dt == torch.float64 else np.int32)).to(device)
    return t


def coarsen_tables(plan, device):
    """The tables of ops.coarsen for a subset.coarsen_plan: its geometry plus device copies of row0 / ntap (int32 [Ho])
    and rw (fp64 [Ho, k_lat + 1])."""
    return _device_tables(plan, plan, _COARSEN_TABLES, device)


def regrid_tables(plan, device):
    """The tables of ops.regrid for a regrid.Grid.plan: its geometry plus device copies of row0 / ntap / order (int32
    [Ho]), rw (fp64 [Ho, Tmax]), col0 / ctap (int32 [Wo]), cw (fp64 [Wo, Umax]) and the column tiles (int32 [n, 4],
    regrid.tile_table: computed here, on the host, for the kernel's LDS budget)."""
    from . import regrid as _rg
    tiles, tile_cols, max_span = _rg.tile_table(plan)
    return _device_tables(dict(plan, tile_cols=tile_cols, max_span=max_span), dict(plan, tiles=tiles), _REGRID_TABLES, device)


def _window_reduce(what, x, t, out, chan_map, launch):
    """The body of ops.coarsen / ops.regrid (`what`; csrc/window_reduce.hip): the device tables `t` against the
    operator's (name, dtype) spec and the plan's Ho / Wo, x against the plan's source box, chan_map, `out` (allocated
    when None), then launch(C, C_out, out, (sr0, Hs, sc0, Ws), (H, W)) inside the timer bracket."""
    spec, origin, belong = _WINDOW_OPS[what]
    _dev(x, out)
    ok = isinstance(t, dict) and all(isinstance(t.get(k), torch.Tensor) and t[k].is_cuda and t[k].is_contiguous()
                                     and t[k].dtype == dt for k, dt in spec)
    if not ok:
        raise ValueError(f"{what}: {origin}")
    Ho, Wo = int(t["Ho"]), int(t["Wo"])
    sr0, sr1, sc0, snc = (int(v) for v in t["src_box"])
    H, W = (int(v) for v in t["grid"])
    if any(t[k].device != x.device for k, _ in spec):
        raise ValueError(f"{what}: the tables are on {t['row0'].device}, x on {x.device}")

    def belongs(k):       # rw / cw are matrices, tiles [n, 4], the others vectors; first dimension Ho (rows) or Wo (columns)
        if k == "tiles":
            return t[k].dim() == 2 and t[k].shape[1] == 4 and t[k].shape[0] >= 1
        return t[k].dim() == (2 if k in ("rw", "cw") else 1) and t[k].shape[0] == (Wo if k in ("col0", "ctap", "cw") else Ho)
    if not all(belongs(k) for k, _ in spec):
        raise ValueError(f"{what}: the tables do not belong to a plan of {belong.format(Ho=Ho, Wo=Wo)}")
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous() or tuple(x.shape[1:]) != (sr1 - sr0, snc):
        raise ValueError(f"{what}: x must be a contiguous fp32 [C, {sr1 - sr0}, {snc}] tensor - the plan's source box "
                         f"{(sr0, sr1, sc0, snc)} (got {tuple(x.shape)} {x.dtype})")
    C = x.shape[0]
    if chan_map is not None:
        if not (isinstance(chan_map, torch.Tensor) and chan_map.is_cuda and chan_map.dtype == torch.int32
                and chan_map.dim() == 1 and chan_map.is_contiguous() and chan_map.numel() > 0
                and chan_map.device == x.device):
            raise ValueError(f"{what}: chan_map must be a contiguous int32 vector on x's device")
        C_out = chan_map.numel()
    else:
        C_out = C
    if out is None:
        out = torch.empty((C_out, Ho, Wo), device=x.device, dtype=torch.float32)
    if not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C_out, Ho, Wo)
            and out.device == x.device):
        raise ValueError(f"{what}: out must be a contiguous fp32 [{C_out}, {Ho}, {Wo}] tensor on x's device")
    with _timed(what, 4.0 * (C_out * (sr1 - sr0) * snc + C_out * Ho * Wo)):
        launch(C, C_out, out, (sr0, sr1 - sr0, sc0, snc), (H, W))
    return out


def coarsen(x, plan_tables, out=None, chan_map=None):
    """cra5_coarsen_f32: the area-weighted mean of x - contiguous fp32 [C, Hs, Ws], the source box plan["src_box"] of an
    H x W global grid - onto the plan's output points -> contiguous fp32 [C_out, Ho, Wo] (`out`, or a fresh tensor).
    plan_tables: coarsen_tables(subset.coarsen_plan(box, k, H, W), device) - the grid (H, W) is the plan's.  chan_map: int32 device [C_out] - output
    channel c is source channel chan_map[c] (a variable subset of a full source needs no gather first); None: C_out = C,
    in order.  The arithmetic is fixed (include/cra5_amd.h): bit-identical from run to run, and a region's result is
    the sub-block of the globe's."""
    t = plan_tables

    def launch(C, C_out, out, src, grid):
        (sr0, Hs, sc0, Ws), (H, W) = src, grid
        ky, kx = (int(v) for v in t["k"])
        check(lib().cra5_coarsen_f32(_p(x), C, Hs, Ws, sr0, sc0, H, W, 1 if (sc0 == 0 and Ws == W) else 0,
                                     int(t["rows"][0]), ky, out.shape[1], int(t["cols"][0]), kx, out.shape[2], _p(t["row0"]),
                                     _p(t["ntap"]), _p(t["rw"]), t["rw"].shape[1], _p(chan_map), C_out, _p(out), _stream()),
              "cra5_coarsen_f32")
    return _window_reduce("coarsen", x, t, out, chan_map, launch)


def regrid(x, tables, out=None, chan_map=None):
    """cra5_regrid_f32: x - contiguous fp32 [C, Hs, Ws], the source box tables["src_box"] of an H x W global grid -
    regridded (bilinear or first-order conservative: the plan's tables) onto the plan's target grid -> contiguous fp32
    [C_out, Ho, Wo] (`out`, or a fresh tensor), rows in the target's own order.  tables: regrid_tables(Grid.plan(H, W),
    device).  chan_map: as in ops.coarsen.  The arithmetic is fixed (include/cra5_amd.h): bit-identical from run to run,
    and a sub-grid's result is the sub-block of the whole target grid's."""
    t = tables

    def launch(C, C_out, out, src, grid):
        (sr0, Hs, sc0, Ws), (H, W) = src, grid
        check(lib().cra5_regrid_f32(_p(x), C, Hs, Ws, sr0, sc0, H, W, out.shape[1], out.shape[2], _p(t["row0"]), _p(t["ntap"]),
                                    _p(t["rw"]), t["rw"].shape[1], _p(t["order"]), _p(t["col0"]), _p(t["ctap"]), _p(t["cw"]),
                                    t["cw"].shape[1], _p(t["tiles"]), t["tiles"].shape[0], int(t["tile_cols"]),
                                    int(t["max_span"]), _p(chan_map), C_out, _p(out), _stream()), "cra5_regrid_f32")
    return _window_reduce("regrid", x, t, out, chan_map, launch)


PROBE_PARTIALS = 256     # CRA5_PROBE_PARTIALS


def probe_sums(x, out, stride=1):
    """cra5_probe_sums_f32: PROBE_PARTIALS partial sums of the flat fp32 tensor `x` (every `stride`-th element) into the
    fp32 device slice `out` [PROBE_PARTIALS]; non-finite anywhere in the sampled elements <=> a non-finite partial."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and out.is_cuda and out.dtype == torch.float32
            and out.is_contiguous() and out.numel() == PROBE_PARTIALS):
        raise TypeError("probe_sums takes a contiguous fp32 device tensor and a contiguous fp32 device slice of PROBE_PARTIALS")
    check(lib().cra5_probe_sums_f32(_p(x), x.numel(), int(stride), _p(out), _stream()), "cra5_probe_sums_f32")
    return out


RECON_FIELDS = ("bias", "mse", "wmse", "mae", "max_abs", "nonfinite")   # CRA5_RECON_* order


def recon_error(x_hat, x, lat_w=None, out=None):
    """cra5_recon_error_f32: per-channel error statistics of x_hat against x (both contiguous fp32 device tensors
    [C, H, W]; lat_w: contiguous fp32 device [H] or None) -> fp64 device tensor [C, len(RECON_FIELDS)] (`out`), in the
    fields of RECON_FIELDS.  On the current stream; the slab of partials comes from torch's caching allocator."""
    ts = (x_hat, x) + ((lat_w,) if lat_w is not None else ())
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        raise TypeError("recon_error takes contiguous fp32 device tensors")
    if x_hat.dim() != 3 or tuple(x_hat.shape) != tuple(x.shape) or x_hat.device != x.device:
        raise ValueError(f"recon_error: x_hat {tuple(x_hat.shape)} and x {tuple(x.shape)} must be [C, H, W] of one shape "
                         "on one device")
    C, H, W = x.shape
    if lat_w is not None and (tuple(lat_w.shape) != (H,) or lat_w.device != x.device):
        raise ValueError(f"recon_error: lat_w must be [{H}] on the frames' device")
    nb = lib().cra5_recon_error_slab_bytes(C, H, W)
    if nb == 0:
        raise ValueError(f"recon_error: unsupported frame shape {(C, H, W)}")
    slab = torch.empty((nb // 8,), device=x.device, dtype=torch.float64)
    if out is None:
        out = torch.empty((C, len(RECON_FIELDS)), device=x.device, dtype=torch.float64)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (C, len(RECON_FIELDS))):
        raise TypeError(f"recon_error: out must be a contiguous fp64 device tensor [{C}, {len(RECON_FIELDS)}]")
    check(lib().cra5_recon_error_f32(_p(x_hat), _p(x), C, H, W, _p(lat_w), _p(slab), nb, _p(out), _stream()),
          "cra5_recon_error_f32")
    return out


PACK_FIELDS = ("vmin", "vmax", "nonfinite", "scale", "offset")   # CRA5_PACK_* order


def _pack_frame(what, x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise TypeError(f"{what} takes a contiguous fp32 device tensor [C, H, W]")
    if x.dim() != 3 or x.numel() == 0 or x.shape[1] * x.shape[2] >= 1 << 31:
        raise ValueError(f"{what}: x {tuple(x.shape)} must be a non-empty [C, H, W] with H * W < 2^31")
    return int(x.shape[0]), int(x.shape[1] * x.shape[2])


def _pack_f64(what, name, t, shape, device):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError(f"{what}: {name} must be a contiguous fp64 device tensor {list(shape)}")
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{what}: {name} must be {list(shape)} on the frame's device, got {tuple(t.shape)} on {t.device}")


def pack_range(x, fixed=None, out=None):
    """cra5_pack_range_f32: per channel of the contiguous fp32 device frame x [C, H, W] the min / max of its finite
    elements, the count of the others and the int16 packing's scale / offset ("Packed int16 output")
    -> fp64 device tensor [C, len(PACK_FIELDS)] (`out`), in the fields of PACK_FIELDS.  fixed: fp64 device [C, 2] (lo, hi)
    or None; a row whose lo is NaN takes the frame's own range, any other row must be finite with lo < hi (the caller's
    duty: pack.resolve_ranges checks it on the host).  On the current stream; the slab of partials comes from torch's
    caching allocator."""
    C, plane = _pack_frame("pack_range", x)
    if fixed is not None:
        _pack_f64("pack_range", "fixed", fixed, (C, 2), x.device)
    if out is None:
        out = torch.empty((C, len(PACK_FIELDS)), device=x.device, dtype=torch.float64)
    else:
        _pack_f64("pack_range", "out", out, (C, len(PACK_FIELDS)), x.device)
    nb = lib().cra5_pack_range_slab_bytes(C, plane)
    slab = torch.empty((nb // 8,), device=x.device, dtype=torch.float64)
    check(lib().cra5_pack_range_f32(_p(x), C, plane, _p(fixed), _p(slab), nb, _p(out), _stream()), "cra5_pack_range_f32")
    return out


def pack_i16(x, table, out=None):
    """cra5_pack_i16_f32: the int16 codes of the contiguous fp32 device frame x [C, H, W] under the scale / offset of
    `table` (pack_range's fp64 device [C, len(PACK_FIELDS)]) -> int16 device tensor shaped like x (`out`): -32768 for a
    non-finite x, else clamp(rint((double(x) - offset) / scale), -32767, 32767).  On the current stream."""
    C, plane = _pack_frame("pack_i16", x)
    _pack_f64("pack_i16", "table", table, (C, len(PACK_FIELDS)), x.device)
    if out is None:
        out = torch.empty(tuple(x.shape), device=x.device, dtype=torch.int16)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int16 and out.is_contiguous()):
        raise TypeError(f"pack_i16: out must be a contiguous int16 device tensor {list(x.shape)}")
    elif tuple(out.shape) != tuple(x.shape) or out.device != x.device:
        raise ValueError(f"pack_i16: out must be {list(x.shape)} on the frame's device, got {tuple(out.shape)} on {out.device}")
    check(lib().cra5_pack_i16_f32(_p(x), C, plane, _p(table), _p(out), _stream()), "cra5_pack_i16_f32")
    return out


UNPACK_FIELDS = ("scale", "offset", "fill", "mul")   # CRA5_UNPACK_* order
UNPACK_SWAPPED = 1                                   # CRA5_UNPACK_SWAPPED


def unpack_i16(q, table, swapped=False, out=None):
    """cra5_unpack_i16_f32: the fp32 values of the contiguous int16 device codes q [C, H, W] under `table` (fp64 device
    [C, len(UNPACK_FIELDS)]: scale, offset, fill code (NaN: none), fp32-exact multiplier) -> fp32 device tensor shaped
    like q (`out`): NaN for the fill code, else float(double(q) * scale + offset) * float(mul), the float64 multiply and
    add rounded separately ("Packed int16 input").  swapped: the codes' bytes are in the other
    order and are swapped in registers.  On the current stream."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.int16 and q.is_contiguous()):
        raise TypeError("unpack_i16 takes a contiguous int16 device tensor [C, H, W]")
    if q.dim() != 3 or q.numel() == 0 or q.shape[1] * q.shape[2] >= 1 << 31:
        raise ValueError(f"unpack_i16: q {tuple(q.shape)} must be a non-empty [C, H, W] with H * W < 2^31")
    C, plane = int(q.shape[0]), int(q.shape[1] * q.shape[2])
    _pack_f64("unpack_i16", "table", table, (C, len(UNPACK_FIELDS)), q.device)
    if out is None:
        out = torch.empty(tuple(q.shape), device=q.device, dtype=torch.float32)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
        raise TypeError(f"unpack_i16: out must be a contiguous fp32 device tensor {list(q.shape)}")
    elif tuple(out.shape) != tuple(q.shape) or out.device != q.device:
        raise ValueError(f"unpack_i16: out must be {list(q.shape)} on the codes' device, got {tuple(out.shape)} on {out.device}")
    check(lib().cra5_unpack_i16_f32(_p(q), C, plane, _p(table), UNPACK_SWAPPED if swapped else 0, _p(out), _stream()),
          "cra5_unpack_i16_f32")
    return out


SPECTRUM_MAX_W = 1440    # CRA5_SPECTRUM_MAX_W
_TWIDDLES = {}           # (W, device) -> fp64 device [W, 2]: (cos, sin) of -2 pi j / W


def spectrum_width_ok(W):
    """W is a width cra5_zonal_spectrum_f32 transforms: 2 <= W <= SPECTRUM_MAX_W with no prime factor above 5."""
    W = int(W)
    if not 2 <= W <= SPECTRUM_MAX_W:
        return False
    for p in (2, 3, 5):
        while W % p == 0:
            W //= p
    return W == 1


def _twiddles(W, device):
    key = (W, str(device))
    t = _TWIDDLES.get(key)
    if t is None:
        a = -2.0 * np.pi * np.arange(W, dtype=np.float64) / W
        t = _TWIDDLES[key] = torch.from_numpy(np.stack([np.cos(a), np.sin(a)], axis=1)).to(device)
    return t


def zonal_spectrum(x_hat, x, lat_w=None, out=None):
    """cra5_zonal_spectrum_f32: zonal power spectra of the truth x, the reconstruction x_hat and d = x_hat - x (both
    contiguous fp32 device tensors [C, H, W]; lat_w: contiguous fp32 device [H] or None) -> (power, nonfinite): fp64
    device tensors [3, C, K] (P_x, P_x_hat, P_d; K = W // 2 + 1) and [C], both views of `out`, one flat fp64 device tensor
    of 3 * C * K + C elements (allocated when None), so that one copy brings everything to the host.  On the current
    stream; the twiddle table is cached per (W, device), the slab of partials comes from torch's caching allocator."""
    ts = (x_hat, x) + ((lat_w,) if lat_w is not None else ())
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        raise TypeError("zonal_spectrum takes contiguous fp32 device tensors")
    if x_hat.dim() != 3 or tuple(x_hat.shape) != tuple(x.shape) or x_hat.device != x.device:
        raise ValueError(f"zonal_spectrum: x_hat {tuple(x_hat.shape)} and x {tuple(x.shape)} must be [C, H, W] of one "
                         "shape on one device")
    C, H, W = x.shape
    if lat_w is not None and (tuple(lat_w.shape) != (H,) or lat_w.device != x.device):
        raise ValueError(f"zonal_spectrum: lat_w must be [{H}] on the frames' device")
    if not spectrum_width_ok(W):
        raise ValueError(f"zonal_spectrum: W = {W} is not supported: the row transform takes 2 <= W <= {SPECTRUM_MAX_W} "
                         "with no prime factor above 5")
    nb = lib().cra5_zonal_spectrum_slab_bytes(C, H, W)
    if nb == 0:
        raise ValueError(f"zonal_spectrum: unsupported frame shape {(C, H, W)}")
    K = W // 2 + 1
    if out is None:
        out = torch.empty((3 * C * K + C,), device=x.device, dtype=torch.float64)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
              and tuple(out.shape) == (3 * C * K + C,) and out.device == x.device):
        raise TypeError(f"zonal_spectrum: out must be a contiguous fp64 tensor [{3 * C * K + C}] on the frames' device")
    slab = torch.empty((nb // 8,), device=x.device, dtype=torch.float64)
    power, nonfinite = out[:3 * C * K].view(3, C, K), out[3 * C * K:]
    check(lib().cra5_zonal_spectrum_f32(_p(x_hat), _p(x), C, H, W, _p(lat_w), _p(_twiddles(W, x.device)), _p(slab), nb,
                                        _p(power), _p(nonfinite), _stream()), "cra5_zonal_spectrum_f32")
    return power, nonfinite


QUANTILE_FIELDS = ("truth", "recon", "abs_error")   # the order of the [C, Q] blocks cra5_frame_quantiles_f32 writes
QUANTILE_MAX_Q = 16                                 # CRA5_QUANTILE_MAX_Q


def frame_quantiles(x_hat, x, row_w, targets, out=None):
    """cra5_frame_quantiles_f32: exact quantiles of the truth x, the reconstruction x_hat and |x_hat - x| (both contiguous
    fp32 device tensors [C, H, W]).  row_w: contiguous int32 device [H] of integer row weights in 0 .. 2^20, or None = all
    1; targets: contiguous int64 device [Q], 1 <= Q <= QUANTILE_MAX_Q, every entry in 1 .. W * sum(row_w) (the caller's
    duty: metrics.quantile_weights / quantile_targets) -> (quantiles, nonfinite): fp64 device tensors [3, C, Q] (in the
    order of QUANTILE_FIELDS, every fp32 result widened exactly) and [C], both views of `out`, one flat fp64 device tensor
    of 3 * C * Q + C elements (allocated when None), so that one copy brings everything to the host.  On the current
    stream; the workspace comes from torch's caching allocator and is initialised by the launcher."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               for t in (x_hat, x)):
        raise TypeError("frame_quantiles takes contiguous fp32 device tensors")
    if x_hat.dim() != 3 or tuple(x_hat.shape) != tuple(x.shape) or x_hat.device != x.device:
        raise ValueError(f"frame_quantiles: x_hat {tuple(x_hat.shape)} and x {tuple(x.shape)} must be [C, H, W] of one "
                         "shape on one device")
    C, H, W = x.shape
    if row_w is not None:
        if not (isinstance(row_w, torch.Tensor) and row_w.is_cuda and row_w.dtype == torch.int32 and row_w.is_contiguous()):
            raise TypeError("frame_quantiles: row_w must be a contiguous int32 device tensor or None")
        if tuple(row_w.shape) != (H,) or row_w.device != x.device:
            raise ValueError(f"frame_quantiles: row_w must be [{H}] on the frames' device")
    if not (isinstance(targets, torch.Tensor) and targets.is_cuda and targets.dtype == torch.int64
            and targets.is_contiguous()):
        raise TypeError("frame_quantiles: targets must be a contiguous int64 device tensor [Q]")
    if targets.dim() != 1 or not 1 <= targets.shape[0] <= QUANTILE_MAX_Q or targets.device != x.device:
        raise ValueError(f"frame_quantiles: targets must be [Q] with 1 <= Q <= {QUANTILE_MAX_Q} on the frames' device "
                         f"(got {tuple(targets.shape)} on {targets.device})")
    Q = int(targets.shape[0])
    nb = lib().cra5_frame_quantiles_ws_bytes(C, H, W, Q)
    if nb == 0:
        raise ValueError(f"frame_quantiles: unsupported frame shape {(C, H, W)}")
    if out is None:
        out = torch.empty((3 * C * Q + C,), device=x.device, dtype=torch.float64)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
              and tuple(out.shape) == (3 * C * Q + C,) and out.device == x.device):
        raise TypeError(f"frame_quantiles: out must be a contiguous fp64 tensor [{3 * C * Q + C}] on the frames' device")
    ws = torch.empty((nb // 8,), device=x.device, dtype=torch.int64)
    check(lib().cra5_frame_quantiles_f32(_p(x_hat), _p(x), C, H, W, _p(row_w), _p(targets), Q, _p(ws), nb, _p(out),
                                         _stream()), "cra5_frame_quantiles_f32")
    return out[:3 * C * Q].view(3, C, Q), out[3 * C * Q:]


RESIDUAL_SPAN = 4096     # CRA5_RESIDUAL_SPAN
RESIDUAL_MAX_TOL = 1e30  # step = 2 * tol must stay finite in fp32


def _residual_frame(what, name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError(f"{what}: {name} must be a contiguous fp32 device tensor")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what}: {name} must be [C, H, W], got {tuple(t.shape)}")


def _residual_array(what, name, t, dtype, device, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{what}: {name} must be a contiguous {dtype} device tensor")
    if t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device}, the frame on {device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {list(t.shape)}")


def residual_tolerance(tol, C, what="residual_quantize"):
    """tol (array-like [C]) -> float32 numpy [C], checked: every entry finite > 0 and <= RESIDUAL_MAX_TOL, or +inf (the
    channel is not corrected)."""
    if isinstance(tol, torch.Tensor):
        tol = tol.detach().cpu().numpy()
    t = np.asarray(tol)
    if t.dtype.kind != "f":
        raise TypeError(f"{what}: tol must be a float array, got dtype {t.dtype}")
    if t.shape != (C,):
        raise ValueError(f"{what}: tol must be [{C}] (one tolerance per channel), got {list(t.shape)}")
    t = np.ascontiguousarray(t, dtype=np.float32)
    ok = (np.isposinf(t) | (np.isfinite(t) & (t > 0) & (t <= np.float32(RESIDUAL_MAX_TOL))))
    if not ok.all():
        c = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{what}: tol[{c}] = {t[c]!r}: a tolerance is finite in (0, {RESIDUAL_MAX_TOL:g}] or +inf "
                         "(channel not corrected)")
    return t


def residual_quantize(x, x_hat, tol):
    """cra5_residual_count_f32 / _scan / _emit_f32 (csrc/residual.hip): the corrections that bring the decode x_hat within
    tol of the truth x.  x, x_hat: contiguous fp32 device tensors [C, H, W] of one shape on one device (C * H * W < 2^32);
    tol: float [C] (numpy / list / tensor; residual_tolerance).  -> (idx, q, eidx, ebits, per_channel): device tensors
    idx int32 [n] (the uint32 bit patterns of the flat global indexes), q int16 [n], eidx int32 [m], ebits int32 [m] (the
    bits of x at the escapes), each ascending in idx, and per_channel, a HOST int64 array [C, 2] of (records, escapes).
    On the current stream; the call waits for the counts (they size the arrays)."""
    what = "residual_quantize"
    _residual_frame(what, "x", x)
    _residual_frame(what, "x_hat", x_hat)
    if tuple(x.shape) != tuple(x_hat.shape) or x.device != x_hat.device:
        raise ValueError(f"{what}: x {tuple(x.shape)} on {x.device} and x_hat {tuple(x_hat.shape)} on {x_hat.device} must "
                         "have one shape on one device")
    C, H, W = x.shape
    spans = lib().cra5_residual_spans(C, H, W)
    if spans == 0:
        raise ValueError(f"{what}: x {(C, H, W)}: a frame needs C * H * W < 2^32 (the indexes are uint32)")
    t = residual_tolerance(tol, C, what)
    dev = x.device
    tol_d = torch.from_numpy(t).to(dev)
    counts = torch.empty((spans, 2), device=dev, dtype=torch.int32)
    offs = torch.empty((spans + 1, 2), device=dev, dtype=torch.int32)
    chan = torch.empty((C, 2), device=dev, dtype=torch.int64)
    with _timed("residual_count", 8.0 * C * H * W):
        check(lib().cra5_residual_count_f32(_p(x), _p(x_hat), _p(tol_d), C, H, W, _p(counts), _stream()), "cra5_residual_count_f32")
    check(lib().cra5_residual_scan(_p(counts), C, H, W, _p(offs), _p(chan), _stream()), "cra5_residual_scan")
    per_channel = chan.cpu().numpy()
    n, m = (int(v) for v in per_channel.sum(axis=0))
    idx = torch.empty((n,), device=dev, dtype=torch.int32)
    q = torch.empty((n,), device=dev, dtype=torch.int16)
    eidx = torch.empty((m,), device=dev, dtype=torch.int32)
    ebits = torch.empty((m,), device=dev, dtype=torch.int32)
    with _timed("residual_emit", 8.0 * C * H * W):
        check(lib().cra5_residual_emit_f32(_p(x), _p(x_hat), _p(tol_d), C, H, W, _p(offs), _p(idx) if n else None,
                                           _p(q) if n else None, n, _p(eidx) if m else None, _p(ebits) if m else None, m,
                                           _stream()), "cra5_residual_emit_f32")
    return idx, q, eidx, ebits, per_channel


def _residual_geometry(what, out, grid, chan_lut, box, stride):
    """-> the 13 geometry arguments of cra5_residual_apply_f32 / _gather_f32 after `out`, checked."""
    _residual_frame(what, "out", out)
    try:
        C, H, W = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: grid must be (C, H, W) of the global frame, got {grid!r}") from None
    if lib().cra5_residual_spans(C, H, W) == 0:
        raise ValueError(f"{what}: grid {(C, H, W)}: a frame needs C * H * W < 2^32")
    Cs, Ho, Wo = out.shape
    if chan_lut is not None:
        _residual_array(what, "chan_lut", chan_lut, torch.int32, out.device, (C,))
    elif Cs != C:
        raise ValueError(f"{what}: out has {Cs} channels, the grid {C}: pass chan_lut")
    r0, r1, c0, nc = (0, H, 0, W) if box is None else (int(v) for v in box)
    sy, sx = (1, 1) if stride is None else (int(v) for v in stride)
    if not (0 <= r0 < r1 <= H and 0 <= c0 < W and 1 <= nc <= W):
        raise ValueError(f"{what}: box {box!r}: need 0 <= r0 < r1 <= {H}, 0 <= c0 < {W}, 1 <= nc <= {W}")
    if sy < 1 or sx < 1 or W % sx:
        raise ValueError(f"{what}: stride {stride!r}: need s_lat >= 1, s_lon >= 1 and {W} % s_lon == 0")
    from .subset import kept_points
    rows, cols = kept_points((r0, r1, c0, nc), (sy, sx), W)
    if (Ho, Wo) != (len(rows), len(cols)):
        raise ValueError(f"{what}: out is [{Cs}, {Ho}, {Wo}], the box / stride keep {len(rows)} rows and {len(cols)} columns")
    return (Cs, Ho, Wo, C, H, W, _p(chan_lut), r0, r1, sy, c0, nc, sx), C


def _residual_records(what, records, device):
    try:
        idx, q, eidx, ebits = records
    except (TypeError, ValueError):
        raise ValueError(f"{what}: records must be (idx, q, eidx, ebits)") from None
    for name, t, dt in (("idx", idx, torch.int32), ("q", q, torch.int16), ("eidx", eidx, torch.int32),
                        ("ebits", ebits, torch.int32)):
        _residual_array(what, f"records.{name}", t, dt, device)
        if t.dim() != 1:
            raise ValueError(f"{what}: records.{name} must be one-dimensional, got {list(t.shape)}")
    if idx.numel() != q.numel() or eidx.numel() != ebits.numel():
        raise ValueError(f"{what}: records: idx / q hold {idx.numel()} / {q.numel()} entries, eidx / ebits {eidx.numel()} / "
                         f"{ebits.numel()}")
    return idx, q, eidx, ebits


def residual_apply(out, records, step, grid, chan_lut=None, box=None, stride=None):
    """cra5_residual_apply_f32: correct the decode's output `out` (contiguous fp32 device tensor [C', Ho, Wo]) IN PLACE.
    records = (idx, q, eidx, ebits) of residual_quantize (global indexes of the frame grid = (C, H, W)); step: contiguous
    fp32 device tensor [C] (2 * tol); chan_lut: int32 device tensor [C], the output channel of every global channel or -1
    (None: out holds every channel in order); box (r0, r1, c0, nc) and stride (s_lat, s_lon) as in subset.kept_points
    (None: the globe / every point).  A record adds fl32(q * step[c]) to its point, an escape stores the truth's bits;
    entries outside `out` are skipped.  On the current stream."""
    what = "residual_apply"
    geom, C = _residual_geometry(what, out, grid, chan_lut, box, stride)
    idx, q, eidx, ebits = _residual_records(what, records, out.device)
    _residual_array(what, "step", step, torch.float32, out.device, (C,))
    n, m = idx.numel(), eidx.numel()
    with _timed("residual_apply", 14.0 * n + 16.0 * m):
        check(lib().cra5_residual_apply_f32(_p(out), *geom, _p(step), _p(idx) if n else None, _p(q) if n else None, n,
                                            _p(eidx) if m else None, _p(ebits) if m else None, m, _stream()),
              "cra5_residual_apply_f32")
    return out


def residual_gather(out, widx, grid, chan_lut=None, box=None, stride=None):
    """cra5_residual_gather_f32: the bits of `out` (geometry as in residual_apply) at the global indexes widx (int32
    device tensor [nw], uint32 bit patterns) -> int32 device tensor [nw, 2]: (1, bits) or (0, 0) for a point outside
    `out`.  On the current stream."""
    what = "residual_gather"
    geom, _ = _residual_geometry(what, out, grid, chan_lut, box, stride)
    _residual_array(what, "widx", widx, torch.int32, out.device)
    if widx.dim() != 1:
        raise ValueError(f"{what}: widx must be one-dimensional, got {list(widx.shape)}")
    nw = widx.numel()
    got = torch.empty((nw, 2), device=out.device, dtype=torch.int32)
    check(lib().cra5_residual_gather_f32(_p(out), *geom, _p(widx) if nw else None, nw, _p(got) if nw else None, _stream()),
          "cra5_residual_gather_f32")
    return got


TIME_ACCUMULATORS = (("sum", torch.float64), ("sumsq", torch.float64), ("min", torch.float32), ("max", torch.float32))


def _time_acc(what, acc, shape, device):
    """The accumulator dict of time_accumulate / time_finish, checked: contiguous device tensors of `shape`."""
    if not isinstance(acc, dict) or not acc or not set(acc) <= {k for k, _ in TIME_ACCUMULATORS}:
        raise ValueError(f"{what}: acc must be a dict with any of 'sum', 'sumsq' (fp64), 'min', 'max' (fp32), at least one "
                         f"(got {sorted(acc) if isinstance(acc, dict) else type(acc).__name__})")
    for k, dt in TIME_ACCUMULATORS:
        t = acc.get(k)
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise TypeError(f"{what}: acc[{k!r}] must be a contiguous {dt} device tensor")
        if tuple(t.shape) != tuple(shape) or t.device != device:
            raise ValueError(f"{what}: acc[{k!r}] is {tuple(t.shape)} on {t.device}, the frame {tuple(shape)} on {device}")
    return [acc.get(k) for k, _ in TIME_ACCUMULATORS]


def time_accumulate(x, acc, first):
    """cra5_time_accumulate_f32: fold the contiguous fp32 device tensor `x` into the accumulators `acc` - a dict with any
    of "sum" / "sumsq" (fp64) and "min" / "max" (fp32), each a contiguous device tensor of x's shape.  first: store
    (sum = x, sumsq = x * x, min = max = x; the accumulators may be uninitialised), else update.  On the current stream;
    consecutive calls on the same accumulators must run one after another on the device."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise TypeError("time_accumulate takes a contiguous fp32 device tensor")
    if x.numel() == 0:
        raise ValueError("time_accumulate: the frame is empty")
    s, q, lo, hi = _time_acc("time_accumulate", acc, x.shape, x.device)
    check(lib().cra5_time_accumulate_f32(_p(x), x.numel(), 1 if first else 0, _p(s), _p(q), _p(lo), _p(hi), _stream()),
          "cra5_time_accumulate_f32")
    return acc


def time_finish(acc, count, ddof=0, want=("mean", "std")):
    """cra5_time_finish_f32 on the accumulators of `count` time_accumulate calls -> {"mean": fp32 device tensor,
    "std": ...} for the names in `want`: mean = sum / count, std = sqrt(max(0, (sumsq - sum * sum / count) /
    (count - ddof))), in fp64, rounded to fp32 at the end.  mean needs acc["sum"], std acc["sum"] and acc["sumsq"];
    count - ddof >= 1.  On the current stream."""
    want = tuple(want)
    if not want or not set(want) <= {"mean", "std"}:
        raise ValueError(f"time_finish: want must name 'mean' and / or 'std' (got {want!r})")
    if not isinstance(acc, dict) or acc.get("sum") is None or ("std" in want and acc.get("sumsq") is None):
        raise ValueError("time_finish: mean needs acc['sum'], std needs acc['sum'] and acc['sumsq']")
    count, ddof = int(count), int(ddof)
    if ddof < 0 or count - ddof < 1:
        raise ValueError(f"time_finish: count - ddof must be >= 1 with ddof >= 0 (count {count}, ddof {ddof})")
    ref = acc["sum"]
    if not (isinstance(ref, torch.Tensor) and ref.is_cuda):
        raise TypeError("time_finish takes device accumulators")
    s, q, _, _ = _time_acc("time_finish", acc, ref.shape, ref.device)
    out = {k: torch.empty(ref.shape, device=ref.device, dtype=torch.float32) for k in want}
    check(lib().cra5_time_finish_f32(ref.numel(), count, ddof, _p(s), _p(q) if "std" in want else None, _p(out.get("mean")),
                                     _p(out.get("std")), _stream()), "cra5_time_finish_f32")
    return out


def transpose(x, out=None):
    _dev(x, out)
    R, Cc = x.shape
    if out is None:
        out = torch.empty((Cc, R), device=x.device, dtype=torch.float32)
    check(lib().cra5_transpose_f32(_p(x), _row_stride(x), _p(out), _row_stride(out), R, Cc, _stream()),
          "cra5_transpose_f32")
    return out


def pixel_shuffle(lin, Hz, Wz, p1, p2, out=None):
    _dev(lin, out)
    F = lin.shape[1]
    Cout = F // (p1 * p2)
    assert lin.is_contiguous() and lin.shape[0] == Hz * Wz
    if out is None:
        out = torch.empty((Cout, Hz * p1, Wz * p2), device=lin.device, dtype=torch.float32)
    check(lib().cra5_pixel_shuffle_f32(_p(lin), _p(out), Hz, Wz, p1, p2, Cout, _stream()), "cra5_pixel_shuffle_f32")
    return out


def conv2d(x, w_split, bias, k, stride, act=None):
    """nn.Conv2d(k, stride, padding=k//2) on one image x [C, H, W] (models/utils.py:128-135): padded patch
    gather -> split-f16 GEMM (+ bias) -> [Cout, Ho, Wo].  w_split: SplitMat of weight.reshape(Cout, -1)."""
    _dev(x, bias)
    C, H, W = x.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    cols = SplitMat.empty(Ho * Wo, C * k * k, x.device)
    check(lib().cra5_conv_im2col_f32(_p(x.contiguous()), _p(cols.data), C, H, W, k, k, stride, stride, p, p, Ho, Wo,
                                     cols.Kp, _stream()), "cra5_conv_im2col_f32")
    tok = gemm_nt_split(cols, w_split, bias=bias)                 # [Ho*Wo, Cout]
    out = transpose(tok).view(w_split.rows, Ho, Wo)
    return unary(out, act) if act else out


def conv_transpose2d(x, w_split, bias, cout, k, stride):
    """nn.ConvTranspose2d(k, stride, padding=k//2, output_padding=stride-1) on x [Cin, Hi, Wi]
    (models/utils.py:138-146).  w_split: SplitMat of weight.reshape(Cin, cout*k*k).t()."""
    _dev(x, bias)
    Cin, Hi, Wi = x.shape
    p = k // 2
    Ho, Wo = (Hi - 1) * stride - 2 * p + k + (stride - 1), (Wi - 1) * stride - 2 * p + k + (stride - 1)
    tok = split_f16(transpose(x.reshape(Cin, Hi * Wi).contiguous()))          # [Hi*Wi, Cin]
    cols = gemm_nt_split(tok, w_split)                                        # [Hi*Wi, cout*k*k]
    out = torch.empty((cout, Ho, Wo), device=x.device, dtype=torch.float32)
    check(lib().cra5_deconv_col2im_f32(_p(cols), _p(bias), _p(out), cout, Hi, Wi, k, k, stride, stride, p, p, Ho, Wo,
                                       _row_stride(cols), _stream()), "cra5_deconv_col2im_f32")
    return out


def unary(x, op, slope=0.01):
    """op: 'relu' | 'leaky_relu' (negative slope `slope`, torch's default 0.01; 0.0 is honoured) | 'abs'."""
    _dev(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    code, sl = {"relu": (2, 0.0), "leaky_relu": (0, slope), "abs": (1, 0.0)}[op]
    check(lib().cra5_unary_f32(_p(x), _p(y), x.numel(), code, float(sl), _stream()), "cra5_unary_f32")
    return y


def gaussian_conditional(scales, means, scale_table, y=None, sym_in=None, want=("idx", "sym", "y_hat"),
                         scale_bound=0.11, lik_bound=1e-9):
    """Fused GC kernel. Returns dict with the requested outputs (flat views shaped like `means`)."""
    _dev(scales, means, scale_table, y, sym_in)
    assert scales.is_contiguous() and means.is_contiguous()
    n = means.numel()
    dev = means.device
    o = {}
    o["idx"] = torch.empty(means.shape, device=dev, dtype=torch.int32) if "idx" in want else None
    o["sym"] = torch.empty(means.shape, device=dev, dtype=torch.int32) if "sym" in want else None
    o["y_hat"] = torch.empty(means.shape, device=dev, dtype=torch.float32) if "y_hat" in want else None
    o["lik"] = torch.empty(means.shape, device=dev, dtype=torch.float32) if "lik" in want else None
    if y is not None:
        assert y.is_contiguous() and y.numel() == n
    if sym_in is not None:
        assert sym_in.is_contiguous() and sym_in.numel() == n and sym_in.dtype == torch.int32
    n_table = 0 if scale_table is None else scale_table.numel()   # no table: no indexes (forward() before update())
    if n_table == 0 and "idx" in want:
        raise ValueError("gaussian_conditional: indexes requested without a scale table (run update())")
    check(lib().cra5_gaussian_conditional_f32(_p(y), _p(sym_in), _p(scales), _p(means), _p(scale_table),
                                              n_table, float(scale_bound), float(lik_bound), _p(o["idx"]),
                                              _p(o["sym"]), _p(o["y_hat"]), _p(o["lik"]), n, _stream()),
          "cra5_gaussian_conditional_f32")
    return {k: v for k, v in o.items() if v is not None}


def entropy_bottleneck(medians, params, z=None, sym_in=None, want=("sym", "z_hat"), lik_bound=1e-9, shape=None, sym_out=None):
    """z / sym_in: [C, n] (channel-major).  sym_out: caller-owned int32 device tensor for the symbols (a slice of a packed
    device -> host record buffer)."""
    _dev(medians, params, z, sym_in)
    src = z if z is not None else sym_in
    C = medians.numel()
    n_per = src.numel() // C
    dev = src.device
    o = {}
    o["sym"] = (sym_out.view(src.shape) if sym_out is not None else torch.empty(src.shape, device=dev, dtype=torch.int32)) if "sym" in want else None
    if sym_out is not None:
        assert sym_out.dtype == torch.int32 and sym_out.is_contiguous() and sym_out.numel() == src.numel()
    o["z_hat"] = torch.empty(src.shape, device=dev, dtype=torch.float32) if "z_hat" in want else None
    o["lik"] = torch.empty(src.shape, device=dev, dtype=torch.float32) if "lik" in want else None
    assert src.is_contiguous()
    check(lib().cra5_entropy_bottleneck_f32(_p(z), _p(sym_in), _p(medians), _p(params), float(lik_bound), _p(o["sym"]),
                                            _p(o["z_hat"]), _p(o["lik"]), C, n_per, _stream()),
          "cra5_entropy_bottleneck_f32")
    return {k: v for k, v in o.items() if v is not None}


def gdn(x, beta_eff, gamma_eff, inverse=False):
    _dev(x, beta_eff, gamma_eff)
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    check(lib().cra5_gdn_f32(_p(x), _p(beta_eff), _p(gamma_eff), _p(y), B, C, HW, int(bool(inverse)), _stream()),
          "cra5_gdn_f32")
    return y


# ------------------------------------------------------------------ host entropy coding


def _np_i32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int32)


def _tables(cdf, cdf_len, offsets):
    """Host CDF tables as contiguous int32 arrays: cdf [n_cdfs, stride], cdf_len [n_cdfs], offsets [n_cdfs].  cdf may
    also be a list of (possibly ragged) rows, as the reference's pybind11 module accepts."""
    if isinstance(cdf, (np.ndarray, torch.Tensor)) and cdf.ndim == 2:
        c = _np_i32(cdf)
    else:
        c = np.zeros((len(cdf), max(len(r) for r in cdf)), dtype=np.int32)
        for i, r in enumerate(cdf):
            c[i, : len(r)] = r
    return c, _np_i32(cdf_len).reshape(-1), _np_i32(offsets).reshape(-1)


def _encoded(name, *args):
    """Calls the native encoder `name`(*args, uint8_t **out, size_t *out_len) -> the malloc'ed stream as bytes."""
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    check(getattr(lib(), name)(*args, ctypes.byref(out), ctypes.byref(n)), name)
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().cra5_free(out)


def rans_encode(symbols, indexes, cdf, cdf_len, offsets):
    """-> bytes. Arguments: int32 arrays (numpy or CPU tensors); cdf is [n_cdfs, stride]."""
    s, i = _np_i32(symbols).reshape(-1), _np_i32(indexes).reshape(-1)
    c, l, o = _tables(cdf, cdf_len, offsets)
    if s.size != i.size:
        raise ValueError("`symbols` and `indexes` should have the same size.")
    return _encoded("cra5_rans_encode_with_indexes", s.ctypes.data, i.ctypes.data, s.size, c.ctypes.data, c.shape[0],
                   c.shape[1], l.ctypes.data, o.ctypes.data)


def rans_resolve_symbols(symbols, indexes, cdf, cdf_len, offsets, out=None):
    """Device side of the resolved encoder: int32 DEVICE tensors symbols / indexes [n], tables
    cdf [n_cdfs, stride], cdf_len, offsets -> (start_range uint32-as-int32 [n], raw [n], esc uint8 [n])."""
    for t in (symbols, indexes, cdf, cdf_len, offsets):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise TypeError("rans_resolve_symbols takes contiguous int32 device tensors")
    n = symbols.numel()
    if indexes.numel() != n:
        raise ValueError("`symbols` and `indexes` should have the same size.")
    if out is None:
        out = (torch.empty(n, device=symbols.device, dtype=torch.int32),
               torch.empty(n, device=symbols.device, dtype=torch.int32),
               torch.empty(n, device=symbols.device, dtype=torch.uint8))
    sr, raw, esc = out
    check(lib().cra5_rans_resolve_symbols_i32(_p(symbols), _p(indexes), n, _p(cdf), cdf.shape[0], cdf.shape[1],
                                              _p(cdf_len), _p(offsets), _p(sr), _p(raw),
                                              ctypes.c_void_p(esc.data_ptr()), _stream()),
          "cra5_rans_resolve_symbols_i32")
    return sr, raw, esc


def rans_encode_resolved(start_range, raw, esc):
    """-> bytes, from HOST arrays (numpy / CPU tensors): start_range, raw 32-bit words, esc uint8."""
    def _np(a, dt):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a).view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else np.ascontiguousarray(a, dtype=dt)
    s, r, e = _np(start_range, np.uint32).reshape(-1), _np(raw, np.uint32).reshape(-1), _np(esc, np.uint8).reshape(-1)
    if not (s.size == r.size == e.size):
        raise ValueError("start_range, raw and esc must have the same size")
    return _encoded("cra5_rans_encode_resolved", s.ctypes.data, r.ctypes.data, e.ctypes.data, s.size)


def rans_decode(data, indexes, cdf, cdf_len, offsets, out=None):
    """-> int32 numpy array of len(indexes) (written into `out`, a contiguous int32 array of that
    size, when given: e.g. the numpy view of a pinned staging tensor)."""
    i = _np_i32(indexes).reshape(-1)
    c, l, o = _tables(cdf, cdf_len, offsets)
    if out is None:
        out = np.empty(i.size, dtype=np.int32)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags.c_contiguous and out.size == i.size):
        raise ValueError("`out` must be a contiguous int32 numpy array with one entry per index")
    buf = (ctypes.c_char * len(data)).from_buffer_copy(data)
    check(lib().cra5_rans_decode_with_indexes(ctypes.addressof(buf), len(data), i.ctypes.data, i.size, c.ctypes.data,
                                              c.shape[0], c.shape[1], l.ctypes.data, o.ctypes.data, out.ctypes.data),
          "cra5_rans_decode_with_indexes")
    return out


def rans_resolve_symbols_compact(symbols, indexes, cdf, cdf_len, offsets, out=None):
    """Device side of the compact resolved encoder -> (start_range int32 [n], rec16 int16 [n], overflow int32 [1]).
    out: caller-owned (sr, rec, ovf) device tensors of those types (slices of a packed record buffer)."""
    for t in (symbols, indexes, cdf, cdf_len, offsets):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise TypeError("rans_resolve_symbols_compact takes contiguous int32 device tensors")
    n = symbols.numel()
    if indexes.numel() != n:
        raise ValueError("`symbols` and `indexes` should have the same size.")
    if out is not None:
        sr, rec, ovf = out
        assert sr.dtype == torch.int32 and rec.dtype == torch.int16 and ovf.dtype == torch.int32
        assert sr.numel() == n and rec.numel() == n and ovf.numel() == 1 and sr.is_contiguous() and rec.is_contiguous()
    else:
        sr = torch.empty(n, device=symbols.device, dtype=torch.int32)
        rec = torch.empty(n, device=symbols.device, dtype=torch.int16)
        ovf = torch.empty(1, device=symbols.device, dtype=torch.int32)
    check(lib().cra5_rans_resolve_symbols_compact(_p(symbols), _p(indexes), n, _p(cdf), cdf.shape[0], cdf.shape[1],
                                                  _p(cdf_len), _p(offsets), _p(sr), ctypes.c_void_p(rec.data_ptr()),
                                                  _p(ovf), _stream()), "cra5_rans_resolve_symbols_compact")
    return sr, rec, ovf


def rans_encode_resolved_compact(start_range, rec16):
    """-> bytes, from HOST arrays: start_range (32-bit words), rec16 (16-bit records)."""
    s_ = np.ascontiguousarray(start_range).view(np.uint32).reshape(-1)
    r_ = np.ascontiguousarray(rec16).view(np.uint16).reshape(-1)
    if s_.size != r_.size:
        raise ValueError("start_range and rec16 must have the same size")
    return _encoded("cra5_rans_encode_resolved_compact", s_.ctypes.data, r_.ctypes.data, s_.size)


def rans_decode_compact(data, indexes_u8, cdf, cdf_len, offsets, out):
    """cra5_rans_decode_with_indexes_u8_i16: uint8 index array -> the int16 numpy array `out` (e.g. the view of a pinned
    staging tensor).  Raises Cra5Error with status ERR_RANGE when a symbol does not fit int16 (decode again with
    rans_decode)."""
    if not (isinstance(indexes_u8, np.ndarray) and indexes_u8.dtype == np.uint8 and indexes_u8.flags.c_contiguous):
        raise ValueError("`indexes_u8` must be a contiguous uint8 numpy array")
    if not (isinstance(out, np.ndarray) and out.dtype == np.int16 and out.flags.c_contiguous and out.size == indexes_u8.size):
        raise ValueError("`out` must be a contiguous int16 numpy array with one entry per index")
    c, l, o = _tables(cdf, cdf_len, offsets)
    buf = (ctypes.c_char * len(data)).from_buffer_copy(data)
    check(lib().cra5_rans_decode_with_indexes_u8_i16(ctypes.addressof(buf), len(data), indexes_u8.ctypes.data,
                                                     indexes_u8.size, c.ctypes.data, c.shape[0], c.shape[1],
                                                     l.ctypes.data, o.ctypes.data, out.ctypes.data),
          "cra5_rans_decode_with_indexes_u8_i16")
    return out


def gaussian_conditional_compact(scales, means, scale_table=None, sym16_in=None, want_idx8=False, scale_bound=0.11, idx8_out=None):
    """Decode-side halves of gaussian_conditional on compact records: want_idx8 -> uint8 CDF indexes (same shape as
    means); sym16_in (int16 device tensor) -> y_hat = sym + mean (fp32).  Returns {"idx8": ..., "y_hat": ...}."""
    _dev(scales, means, scale_table, sym16_in)
    n = means.numel()
    out = {}
    idx8 = (idx8_out if idx8_out is not None else torch.empty(means.shape, device=means.device, dtype=torch.uint8)) if want_idx8 else None
    if idx8_out is not None:
        assert idx8_out.dtype == torch.uint8 and idx8_out.is_contiguous() and idx8_out.numel() == n
    y_hat = torch.empty(means.shape, device=means.device, dtype=torch.float32) if sym16_in is not None else None
    if sym16_in is not None:
        assert sym16_in.dtype == torch.int16 and sym16_in.is_contiguous() and sym16_in.numel() == n
    assert means.is_contiguous() and (scales is None or scales.is_contiguous())
    check(lib().cra5_gaussian_conditional_compact_f32(
        _p(scales), _p(means), _p(scale_table), scale_table.numel() if scale_table is not None else 0, float(scale_bound),
        ctypes.c_void_p(sym16_in.data_ptr()) if sym16_in is not None else None,
        ctypes.c_void_p(idx8.data_ptr()) if idx8 is not None else None, _p(y_hat), n, _stream()),
          "cra5_gaussian_conditional_compact_f32")
    if idx8 is not None:
        out["idx8"] = idx8
    if y_hat is not None:
        out["y_hat"] = y_hat
    return out


def pmf_to_quantized_cdf(pmf, precision=16):
    p = np.ascontiguousarray(np.asarray(pmf, dtype=np.float32))
    out = np.empty(p.size + 1, dtype=np.uint32)
    rc = lib().cra5_pmf_to_quantized_cdf(p.ctypes.data, p.size, precision, out.ctypes.data)
    if rc in (-3, -4, -5):
        raise ValueError({-3: "Invalid `pmf`, non-finite or negative element found",
                          -4: "Invalid `pmf`: at least one element must have a non-zero probability.",
                          -5: "Invalid `pmf`: no bin can donate frequency"}[rc])
    check(rc, "cra5_pmf_to_quantized_cdf")
    return out
