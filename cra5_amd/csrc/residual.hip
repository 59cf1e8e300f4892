// Error-bounded residual layer ("Residual layer"): quantised corrections of a decode against its truth.
//
// Per point of a corrected channel (tol finite), x the truth and h the plain decode, in float64 unless said otherwise:
//   d = x - h,  q = rint(d / step)  (step = fp32 2 * tol, ties to even);  d not finite or |q| > 32767: ESCAPE;
//   t = h for q == 0, else t = fl32(h + fl32((float)q * step)) - two separately rounded fp32 operations;
//   |x - t| <= tol: accepted (q != 0: a RECORD (idx, q); q == 0: nothing), otherwise an ESCAPE (idx, the bits of x).
//
// Quantise = deterministic two-pass compaction.  The frame is cut into spans of kSpan elements that never straddle a
// channel; residual_count_kernel writes the (records, escapes) of every span, residual_scan_kernel (one block) turns them
// into exclusive offsets and per-channel totals, residual_emit_kernel classifies the span again - no frame-sized temporary -
// and stores its entries at those offsets.  Inside a span the order is (pass u, wave, lane, component j) = ascending element
// index: positions come from wave64 ballots / popcounts and per-(pass, wave) totals in LDS.  No atomics anywhere: the
// arrays are identical from run to run.
//
// Apply = one thread per record / escape, mapped from the GLOBAL index into the decode's output [C'][Ho][Wo], which may be a
// channel subset, a box and a stride (subset.kept_points).  No two entries share an index: plain stores, no atomics.
// The fp32 correction is TWO roundings, fl32(h + fl32(q * step)): no FMA contraction anywhere in this file (hipcc's default
// is -ffp-contract=fast, and the runtime's __fmul_rn / __fadd_rn are plain operators that it would fuse as well).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPasses = 4;                          // float4 quads per thread and span
constexpr int kSpan = CRA5_RESIDUAL_SPAN;           // kThreads * 4 * kPasses elements
static_assert(kSpan == kThreads * 4 * kPasses, "span = threads x quad x passes");
constexpr int kScanThreads = 1024;

enum : int { kNone = 0, kRecord = 1, kEscape = 2 };

// -> kNone / kRecord / kEscape, *q the record's value.  |d| <= tol <=> q == 0 exactly (step = 2 tol is exact, 0.5 and its
// upper neighbour are doubles, division rounds monotonically), and q == 0 is always accepted: the common point costs no
// division.  A NaN d fails the comparison and reaches the finiteness test.
__device__ __forceinline__ int classify(float x, float h, float tol, float step, int *q) {
  const double d = (double)x - (double)h;
  if (fabs(d) <= (double)tol) return kNone;
  if ((__double_as_longlong(d) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll) return kEscape;
  const double qd = rint(d / (double)step);
  if (!(fabs(qd) <= 32767.0)) return kEscape;
  const int qi = (int)qd;
  *q = qi;
  const float p = (float)qi * step;      // (contract(off): a multiply, then an add)
  const float t = qi == 0 ? h : h + p;
  const double e = fabs((double)x - (double)t);
  if (!(e <= (double)tol)) return kEscape;
  return qi == 0 ? kNone : kRecord;
}

__device__ __forceinline__ bool corrected(float tol) { return tol > 0.f && tol < INFINITY; }

struct Quad {
  float x[4], h[4];
  int n;      // elements of the quad inside the span
};

// quad (u, tid) of the span starting at element g0 (len elements): 16-byte loads where `vec`, else element by element
__device__ __forceinline__ Quad load_quad(const float *__restrict__ x, const float *__restrict__ xh, size_t g0, int len,
                                          int u, int tid, bool vec) {
  Quad v;
  const int e = (u * kThreads + tid) * 4;
  v.n = min(4, max(0, len - e));
  if (vec && v.n == 4) {
    const float4 a = *reinterpret_cast<const float4 *>(x + g0 + e);
    const float4 b = *reinterpret_cast<const float4 *>(xh + g0 + e);
    v.x[0] = a.x, v.x[1] = a.y, v.x[2] = a.z, v.x[3] = a.w;
    v.h[0] = b.x, v.h[1] = b.y, v.h[2] = b.z, v.h[3] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v.x[j] = j < v.n ? x[g0 + e + j] : 0.f;
      v.h[j] = j < v.n ? xh[g0 + e + j] : 0.f;
    }
  }
  return v;
}

struct SpanGeom {
  int c, len;
  size_t g0;
  bool vec;
};

__device__ __forceinline__ SpanGeom span_geom(const float *x, const float *xh, int HW, int spans_per_chan) {
  SpanGeom s;
  s.c = blockIdx.x / spans_per_chan;
  const int k = blockIdx.x - s.c * spans_per_chan;
  s.len = min(kSpan, HW - k * kSpan);
  s.g0 = (size_t)s.c * HW + (size_t)k * kSpan;
  s.vec = ((uintptr_t)(x + s.g0) % 16) == 0 && ((uintptr_t)(xh + s.g0) % 16) == 0;
  return s;
}

// counts [spans][2] = (records, escapes) of every span; a channel that is not corrected writes zeros
__global__ __launch_bounds__(kThreads) void residual_count_kernel(const float *__restrict__ x, const float *__restrict__ xh,
                                                                  const float *__restrict__ tol, int HW, int spans_per_chan,
                                                                  uint32_t *__restrict__ counts) {
  __shared__ uint32_t red[kWaves][2];
  const SpanGeom s = span_geom(x, xh, HW, spans_per_chan);
  const int tid = threadIdx.x;
  const float t = tol[s.c];
  if (!corrected(t)) {     // (uniform over the block)
    if (tid < 2) counts[(size_t)blockIdx.x * 2 + tid] = 0u;
    return;
  }
  const float step = 2.f * t;
  Quad v[kPasses];
#pragma unroll
  for (int u = 0; u < kPasses; ++u) v[u] = load_quad(x, xh, s.g0, s.len, u, tid, s.vec);
  uint32_t nr = 0, ne = 0;
#pragma unroll
  for (int u = 0; u < kPasses; ++u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int q;
      const int kind = j < v[u].n ? classify(v[u].x[j], v[u].h[j], t, step, &q) : kNone;
      nr += kind == kRecord;
      ne += kind == kEscape;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nr += __shfl_xor(nr, off, 64);
    ne += __shfl_xor(ne, off, 64);
  }
  if ((tid & 63) == 0) red[tid >> 6][0] = nr, red[tid >> 6][1] = ne;
  __syncthreads();
  if (tid < 2) {
    uint32_t a = 0;
    for (int w = 0; w < kWaves; ++w) a += red[w][tid];
    counts[(size_t)blockIdx.x * 2 + tid] = a;
  }
}

// ONE block: offs [spans + 1][2] = exclusive prefix sums of counts (the last row: the totals), chan [C][2] = the totals
// of every channel.  Thread t owns a contiguous run of spans; the kScanThreads run totals are scanned through LDS.
__global__ __launch_bounds__(kScanThreads) void residual_scan_kernel(const uint32_t *__restrict__ counts, int spans,
                                                                     int spans_per_chan, int C, uint32_t *__restrict__ offs,
                                                                     long long *__restrict__ chan) {
  __shared__ uint32_t part[kScanThreads][2];
  const int tid = threadIdx.x;
  const int per = (spans + kScanThreads - 1) / kScanThreads;
  const int b = min(spans, tid * per), e = min(spans, b + per);
  uint32_t a0 = 0, a1 = 0;
  for (int i = b; i < e; ++i) a0 += counts[2 * (size_t)i], a1 += counts[2 * (size_t)i + 1];
  part[tid][0] = a0, part[tid][1] = a1;
  __syncthreads();
  // Hillis-Steele inclusive scan over the run totals (10 rounds; this kernel is microseconds)
  for (int off = 1; off < kScanThreads; off <<= 1) {
    uint32_t p0 = 0, p1 = 0;
    if (tid >= off) p0 = part[tid - off][0], p1 = part[tid - off][1];
    __syncthreads();
    part[tid][0] += p0, part[tid][1] += p1;
    __syncthreads();
  }
  uint32_t r0 = part[tid][0] - a0, r1 = part[tid][1] - a1;      // exclusive
  for (int i = b; i < e; ++i) {
    offs[2 * (size_t)i] = r0, offs[2 * (size_t)i + 1] = r1;
    r0 += counts[2 * (size_t)i], r1 += counts[2 * (size_t)i + 1];
  }
  if (tid == kScanThreads - 1) offs[2 * (size_t)spans] = part[tid][0], offs[2 * (size_t)spans + 1] = part[tid][1];
  __syncthreads();      // (the block's own global stores are visible to it after the barrier)
  for (int c = tid; c < C; c += kScanThreads) {
    const size_t lo = (size_t)c * spans_per_chan, hi = lo + spans_per_chan;
    chan[2 * (size_t)c] = (long long)(offs[2 * hi] - offs[2 * lo]);
    chan[2 * (size_t)c + 1] = (long long)(offs[2 * hi + 1] - offs[2 * lo + 1]);
  }
}

// idx / q [n], eidx / ebits [m]: the entries of every span at its scanned offset, ascending inside the span
__global__ __launch_bounds__(kThreads) void residual_emit_kernel(const float *__restrict__ x, const float *__restrict__ xh,
                                                                 const float *__restrict__ tol, int HW, int spans_per_chan,
                                                                 const uint32_t *__restrict__ offs, uint32_t *__restrict__ idx,
                                                                 int16_t *__restrict__ qv, uint32_t n,
                                                                 uint32_t *__restrict__ eidx, uint32_t *__restrict__ ebits,
                                                                 uint32_t m) {
  __shared__ uint32_t tot[kPasses][kWaves][2];
  const SpanGeom s = span_geom(x, xh, HW, spans_per_chan);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float t = tol[s.c];
  if (!corrected(t)) return;      // (uniform over the block)
  const uint32_t base_r = offs[2 * (size_t)blockIdx.x], base_e = offs[2 * (size_t)blockIdx.x + 1];
  if (offs[2 * (size_t)blockIdx.x + 2] == base_r && offs[2 * (size_t)blockIdx.x + 3] == base_e) return;   // an empty span
  const float step = 2.f * t;
  Quad v[kPasses];
#pragma unroll
  for (int u = 0; u < kPasses; ++u) v[u] = load_quad(x, xh, s.g0, s.len, u, tid, s.vec);
  const unsigned long long below = (1ull << lane) - 1ull;
  int kind[kPasses][4], q[kPasses][4];
  uint32_t pos_r[kPasses], pos_e[kPasses];      // this thread's first position inside (pass, wave)
#pragma unroll
  for (int u = 0; u < kPasses; ++u) {
    uint32_t pr = 0, pe = 0, wr = 0, we = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q[u][j] = 0;
      kind[u][j] = j < v[u].n ? classify(v[u].x[j], v[u].h[j], t, step, &q[u][j]) : kNone;
      const unsigned long long br = __ballot(kind[u][j] == kRecord), be = __ballot(kind[u][j] == kEscape);
      pr += __popcll(br & below), pe += __popcll(be & below);
      wr += __popcll(br), we += __popcll(be);
    }
    pos_r[u] = pr, pos_e[u] = pe;
    if (lane == 0) tot[u][wave][0] = wr, tot[u][wave][1] = we;
  }
  __syncthreads();
  uint32_t run_r = base_r, run_e = base_e;
#pragma unroll
  for (int u = 0; u < kPasses; ++u) {
    uint32_t at_r = run_r, at_e = run_e;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) at_r += tot[u][w][0], at_e += tot[u][w][1];
      run_r += tot[u][w][0], run_e += tot[u][w][1];
    }
    uint32_t o_r = at_r + pos_r[u], o_e = at_e + pos_e[u];
    const uint32_t g = (uint32_t)(s.g0 + (size_t)(u * kThreads + tid) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kind[u][j] == kRecord) {
        if (o_r < n) idx[o_r] = g + j, qv[o_r] = (int16_t)q[u][j];
        ++o_r;
      } else if (kind[u][j] == kEscape) {
        if (o_e < m) eidx[o_e] = g + j, ebits[o_e] = __float_as_uint(v[u].x[j]);
        ++o_e;
      }
    }
  }
}

struct Geom {
  int C, H, W, Cs, Ho, Wo;
  int r0, r1, sy, rfirst;      // rows [r0, r1) with r % sy == 0; rfirst: the first kept one
  int c0, nc, sx, f;           // columns c0 .. c0 + nc - 1 (mod W) with col % sx == 0; f: box offset of the first kept one
  const int *lut;              // [C]: output channel or -1; NULL: the identity
};

// global index -> element offset in the output [Cs][Ho][Wo], or -1 when the point is not in it
__device__ __forceinline__ long long locate(uint32_t i, const Geom &g) {
  const uint32_t HW = (uint32_t)g.H * (uint32_t)g.W;
  const uint32_t c = i / HW;
  if (c >= (uint32_t)g.C) return -1;
  const uint32_t l = i - c * HW, r = l / (uint32_t)g.W, col = l - r * (uint32_t)g.W;
  const int cs = g.lut ? g.lut[c] : (int)c;
  if (cs < 0 || cs >= g.Cs) return -1;
  if ((int)r < g.r0 || (int)r >= g.r1 || r % (uint32_t)g.sy) return -1;
  int k = (int)col - g.c0;
  if (k < 0) k += g.W;
  if (k >= g.nc || col % (uint32_t)g.sx) return -1;
  const int orow = ((int)r - g.rfirst) / g.sy, ocol = (k - g.f) / g.sx;
  if (orow < 0 || orow >= g.Ho || k < g.f || ocol >= g.Wo) return -1;
  return ((long long)cs * g.Ho + orow) * g.Wo + ocol;
}

__global__ __launch_bounds__(kThreads) void residual_apply_records_kernel(float *__restrict__ out, Geom g,
                                                                          const float *__restrict__ step,
                                                                          const uint32_t *__restrict__ idx,
                                                                          const int16_t *__restrict__ qv, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = idx[i];
  const long long o = locate(id, g);
  if (o < 0) return;
  const float s = step[id / ((uint32_t)g.H * (uint32_t)g.W)];
  const float p = (float)qv[i] * s;      // (contract(off): a multiply, then an add)
  out[o] = out[o] + p;
}

__global__ __launch_bounds__(kThreads) void residual_apply_escapes_kernel(float *__restrict__ out, Geom g,
                                                                          const uint32_t *__restrict__ eidx,
                                                                          const uint32_t *__restrict__ ebits, uint32_t m) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (i >= m) return;
  const long long o = locate(eidx[i], g);
  if (o < 0) return;
  out[o] = __uint_as_float(ebits[i]);
}

// got [2 * nw]: (1, the bits of out at witness i) when the witness lies in the output, else (0, 0)
__global__ __launch_bounds__(kThreads) void residual_gather_kernel(const float *__restrict__ out, Geom g,
                                                                   const uint32_t *__restrict__ widx, uint32_t nw,
                                                                   uint32_t *__restrict__ got) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (i >= nw) return;
  const long long o = locate(widx[i], g);
  got[2 * (size_t)i] = o >= 0 ? 1u : 0u;
  got[2 * (size_t)i + 1] = o >= 0 ? __float_as_uint(out[o]) : 0u;
}

bool frame_ok(int C, int H, int W) {
  return C > 0 && H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu && (size_t)C * H * W <= 0xffffffffull;
}

int spans_per_chan(int H, int W) { return (int)(((size_t)H * W + kSpan - 1) / kSpan); }

bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

// the kept rows / columns of (box, stride) must be exactly Ho x Wo (subset.kept_points)
bool make_geom(Geom &g, int Cs, int Ho, int Wo, int C, int H, int W, const int *lut, int r0, int r1, int sy, int c0, int nc,
               int sx) {
  if (!frame_ok(C, H, W) || Cs <= 0 || Ho <= 0 || Wo <= 0 || (size_t)Cs * Ho * Wo > 0x7fffffffffffull) return false;
  if (!(0 <= r0 && r0 < r1 && r1 <= H && 0 <= c0 && c0 < W && 1 <= nc && nc <= W && sy >= 1 && sx >= 1 && W % sx == 0))
    return false;
  const int rfirst = (r0 + sy - 1) / sy * sy;
  const int f = (sx - c0 % sx) % sx;
  if (rfirst >= r1 || f >= nc) return false;
  if ((r1 - 1 - rfirst) / sy + 1 != Ho || (nc - 1 - f) / sx + 1 != Wo) return false;
  g = Geom{C, H, W, Cs, Ho, Wo, r0, r1, sy, rfirst, c0, nc, sx, f, lut};
  return true;
}

}  // namespace

extern "C" {

size_t cra5_residual_spans(int C, int H, int W) {
  if (!frame_ok(C, H, W)) return 0;
  const size_t n = (size_t)C * spans_per_chan(H, W);
  return n <= 0x3fffffffu ? n : 0;
}

int cra5_residual_count_f32(const float *x, const float *x_hat, const float *tol, int C, int H, int W, uint32_t *counts,
                            void *stream) {
  const size_t spans = cra5_residual_spans(C, H, W);
  if (!x || !x_hat || !tol || !counts || !spans) return CRA5_ERR_ARG;
  if (!aligned(x, 4) || !aligned(x_hat, 4) || !aligned(tol, 4) || !aligned(counts, 4)) return CRA5_ERR_ARG;
  hipLaunchKernelGGL(residual_count_kernel, dim3((unsigned)spans), dim3(kThreads), 0, (hipStream_t)stream, x, x_hat, tol,
                     H * W, spans_per_chan(H, W), counts);
  return (int)hipGetLastError();
}

int cra5_residual_scan(const uint32_t *counts, int C, int H, int W, uint32_t *offs, long long *chan, void *stream) {
  const size_t spans = cra5_residual_spans(C, H, W);
  if (!counts || !offs || !chan || !spans) return CRA5_ERR_ARG;
  if (!aligned(counts, 4) || !aligned(offs, 4) || !aligned(chan, 8)) return CRA5_ERR_ARG;
  hipLaunchKernelGGL(residual_scan_kernel, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, counts, (int)spans,
                     spans_per_chan(H, W), C, offs, chan);
  return (int)hipGetLastError();
}

int cra5_residual_emit_f32(const float *x, const float *x_hat, const float *tol, int C, int H, int W, const uint32_t *offs,
                           uint32_t *idx, int16_t *q, size_t n, uint32_t *eidx, uint32_t *ebits, size_t m, void *stream) {
  const size_t spans = cra5_residual_spans(C, H, W);
  if (!x || !x_hat || !tol || !offs || !spans) return CRA5_ERR_ARG;
  if (n > 0xffffffffull || m > 0xffffffffull || (n && (!idx || !q)) || (m && (!eidx || !ebits))) return CRA5_ERR_ARG;
  if (!aligned(x, 4) || !aligned(x_hat, 4) || !aligned(tol, 4) || !aligned(offs, 4) || !aligned(idx, 4) || !aligned(q, 2) ||
      !aligned(eidx, 4) || !aligned(ebits, 4))
    return CRA5_ERR_ARG;
  if (n == 0 && m == 0) return CRA5_OK;      // nothing to write: no launch
  hipLaunchKernelGGL(residual_emit_kernel, dim3((unsigned)spans), dim3(kThreads), 0, (hipStream_t)stream, x, x_hat, tol,
                     H * W, spans_per_chan(H, W), offs, idx, q, (uint32_t)n, eidx, ebits, (uint32_t)m);
  return (int)hipGetLastError();
}

int cra5_residual_apply_f32(float *out, int Cs, int Ho, int Wo, int C, int H, int W, const int *chan_lut, int r0, int r1,
                            int s_lat, int c0, int nc, int s_lon, const float *step, const uint32_t *idx, const int16_t *q,
                            size_t n, const uint32_t *eidx, const uint32_t *ebits, size_t m, void *stream) {
  Geom g;
  if (!out || !make_geom(g, Cs, Ho, Wo, C, H, W, chan_lut, r0, r1, s_lat, c0, nc, s_lon)) return CRA5_ERR_ARG;
  if (n > 0xffffffffull || m > 0xffffffffull || (n && (!idx || !q || !step)) || (m && (!eidx || !ebits))) return CRA5_ERR_ARG;
  if (!aligned(out, 4) || !aligned(chan_lut, 4) || !aligned(step, 4) || !aligned(idx, 4) || !aligned(q, 2) ||
      !aligned(eidx, 4) || !aligned(ebits, 4))
    return CRA5_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n)
    hipLaunchKernelGGL(residual_apply_records_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       out, g, step, idx, q, (uint32_t)n);
  if (m)
    hipLaunchKernelGGL(residual_apply_escapes_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       out, g, eidx, ebits, (uint32_t)m);
  return (int)hipGetLastError();
}

int cra5_residual_gather_f32(const float *out, int Cs, int Ho, int Wo, int C, int H, int W, const int *chan_lut, int r0,
                             int r1, int s_lat, int c0, int nc, int s_lon, const uint32_t *widx, size_t nw, uint32_t *got,
                             void *stream) {
  Geom g;
  if (!out || !make_geom(g, Cs, Ho, Wo, C, H, W, chan_lut, r0, r1, s_lat, c0, nc, s_lon)) return CRA5_ERR_ARG;
  if (nw > 0xffffffffull || (nw && (!widx || !got))) return CRA5_ERR_ARG;
  if (!aligned(out, 4) || !aligned(chan_lut, 4) || !aligned(widx, 4) || !aligned(got, 4)) return CRA5_ERR_ARG;
  if (nw)
    hipLaunchKernelGGL(residual_gather_kernel, dim3((unsigned)((nw + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, out, g, widx, (uint32_t)nw, got);
  return (int)hipGetLastError();
}

}  // extern "C"
