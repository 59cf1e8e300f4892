// Zonal power spectra of a frame pair: truth x, reconstruction x_hat and their fp32 difference d (cra5_zonal_spectrum_f32).
//
// Pass 1 (spectrum_partials_kernel): one block per (channel, band of rows).  Per row the x and x_hat values are loaded once
// (float4 where the rows are 16-byte aligned; the next row's loads are issued before the current row is transformed) and
// widened to float64 in LDS; d stays in registers.  Two real rows share one complex transform, z = a + i b, A(k) = (Z(k) +
// conj Z(W - k)) / 2, B(k) = (Z(k) - conj Z(W - k)) / 2i: a row's (x, x_hat) is one pair, the d rows of two neighbouring
// latitudes the other - three transforms per two rows.  The transform is a Stockham (self-sorting) mixed-radix FFT,
// radices 4, 2, 3, 5, in float64 between two LDS buffers, with twiddles from the caller's table e^(-2 pi i j / W) (copied
// to LDS once per block where half of it - an even W - or all of it fits beside the buffers).  Every thread keeps the bins
// k = tid, tid + 256, tid + 512 of the three spectra in registers and adds L(h) |F(k)|^2 row after row, then writes the
// band's partial [3][K] and its count of non-finite pairs to the caller's slab.  Plain stores: no memset, no atomics.
// Pass 2 (spectrum_finish_kernel): one thread per (spectrum, k) sums the bands in order and applies m_k / (H W^2) and the
// non-finite flag.  Both passes have a fixed order of operations: the result is bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxW = CRA5_SPECTRUM_MAX_W;
constexpr int kMaxK = kMaxW / 2 + 1;
constexpr int kBins = (kMaxK + kThreads - 1) / kThreads;   // bins of one spectrum per thread
constexpr int kBandRows = 64;                              // even: a pair of d rows never straddles two bands
constexpr int kMaxPasses = 12;
constexpr int kVec = (kMaxW / 4 + kThreads - 1) / kThreads;   // float4 per thread and row
constexpr int kScalar = (kMaxW + kThreads - 1) / kThreads;    // points per thread and row, element by element
constexpr int kElems = 4 * kVec > kScalar ? 4 * kVec : kScalar;

static_assert(kBins * kThreads >= kMaxK, "every bin needs an owner");
// two complex float64 rows (ping-pong), half a twiddle table, the band's weights: two blocks fit a CU's 160 KB
static_assert(2 * kMaxW * 16 + (kMaxW / 2) * 16 + kBandRows * 8 + 64 <= 64 * 1024, "LDS budget per block");

struct Plan {
  int n;
  int radix[kMaxPasses];
};

// W = 2^a 3^b 5^c -> passes of radix 4 .. 4, 2, 3 .. 3, 5 .. 5; false for any other W
bool make_plan(int W, Plan &p) {
  p.n = 0;
  if (W < 2 || W > kMaxW) return false;
  int w = W;
  const int order[4] = {4, 2, 3, 5};
  for (int r : order)
    while (w % r == 0) {
      if (p.n == kMaxPasses) return false;
      p.radix[p.n++] = r;
      w /= r;
    }
  return w == 1;
}

__host__ __device__ inline bool finite_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = v;
  return (c.u & 0x7f800000u) != 0x7f800000u;
}

struct cplx {
  double re, im;
};

__host__ __device__ inline cplx operator+(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ inline cplx operator-(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__host__ __device__ inline cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__host__ __device__ inline cplx mul_neg_i(cplx a) { return {a.im, -a.re}; }   // a * (-i)

// in-place DFT of R points, forward sign e^(-2 pi i j k / R)
template <int R>
__host__ __device__ inline void dft(cplx *v);

template <>
__host__ __device__ inline void dft<2>(cplx *v) {
  const cplx a = v[0];
  v[0] = a + v[1];
  v[1] = a - v[1];
}

template <>
__host__ __device__ inline void dft<4>(cplx *v) {
  const cplx s02 = v[0] + v[2], d02 = v[0] - v[2], s13 = v[1] + v[3], d13 = mul_neg_i(v[1] - v[3]);
  v[0] = s02 + s13;
  v[1] = d02 + d13;
  v[2] = s02 - s13;
  v[3] = d02 - d13;
}

template <>
__host__ __device__ inline void dft<3>(cplx *v) {
  constexpr double s = 0.86602540378443864676;   // sin(2 pi / 3)
  const cplx t = v[1] + v[2], u = v[1] - v[2];
  const cplx m = {v[0].re - 0.5 * t.re, v[0].im - 0.5 * t.im};
  const cplx r = {s * u.im, -s * u.re};          // -i s u
  v[0] = v[0] + t;
  v[1] = m + r;
  v[2] = m - r;
}

template <>
__host__ __device__ inline void dft<5>(cplx *v) {
  constexpr double c1 = 0.30901699437494742410, s1 = 0.95105651629515357212;    // cos, sin of 2 pi / 5
  constexpr double c2 = -0.80901699437494742410, s2 = 0.58778525229247312917;   // cos, sin of 4 pi / 5
  const cplx a = v[1] + v[4], b = v[1] - v[4], c = v[2] + v[3], d = v[2] - v[3];
  const cplx m1 = {v[0].re + c1 * a.re + c2 * c.re, v[0].im + c1 * a.im + c2 * c.im};
  const cplx m2 = {v[0].re + c2 * a.re + c1 * c.re, v[0].im + c2 * a.im + c1 * c.im};
  const cplx t1 = {s1 * b.re + s2 * d.re, s1 * b.im + s2 * d.im};
  const cplx t2 = {s2 * b.re - s1 * d.re, s2 * b.im - s1 * d.im};
  const cplx r1 = mul_neg_i(t1), r2 = mul_neg_i(t2);
  v[0] = v[0] + a + c;
  v[1] = m1 + r1;
  v[4] = m1 - r1;
  v[2] = m2 + r2;
  v[3] = m2 - r2;
}

// The twiddle e^(-2 pi i i / W) from a table of its first `half` entries: the whole table (half = W), or its first half
// for an even W (half = W / 2: the rest is the negation).
__host__ __device__ inline cplx twiddle(const cplx *tw, int half, int i) {
  const bool neg = i >= half;
  const cplx t = tw[neg ? i - half : i];
  return neg ? cplx{-t.re, -t.im} : t;
}

// Butterfly j (0 <= j < W / R) of one Stockham pass: ns = the product of the radices of the earlier passes.  Reads
// in[j + r W / R], writes out[(j / ns) ns R + j % ns + r ns], r < R: every index is below W.
template <int R>
__host__ __device__ inline void bfly_load(const cplx *in, int W, int j, cplx *v) {
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = in[j + r * (W / R)];
}

template <int R>
__host__ __device__ inline void bfly_compute(const cplx *tw, int half, int W, int ns, int k, cplx *v) {
  if (ns > 1) {
    const int step = k * (W / (ns * R));   // r * step <= (R - 1) (ns - 1) W / (ns R) < W
#pragma unroll
    for (int r = 1; r < R; ++r) v[r] = cmul(v[r], twiddle(tw, half, r * step));
  }
  dft<R>(v);
}

template <int R>
__host__ __device__ inline void bfly_store(cplx *out, int ns, int j, int k, const cplx *v) {
  const int o = (j - k) * R + k;
#pragma unroll
  for (int r = 0; r < R; ++r) out[o + r * ns] = v[r];
}

// thread `tid` of `threads`: its butterflies of the pass, two at a time (both loaded before either is computed, so that
// the second one's LDS and twiddle latencies hide behind the first)
template <int R>
__host__ __device__ inline void run_pass(const cplx *in, cplx *out, const cplx *tw, int half, int W, int ns, int tid,
                                         int threads) {
  const int q = W / R;
  for (int j = tid; j < q; j += 2 * threads) {
    const int j1 = j + threads;
    const bool two = j1 < q;
    const int k = j % ns, k1 = j1 % ns;
    cplx a[R], b[R];
    bfly_load<R>(in, W, j, a);
    if (two) bfly_load<R>(in, W, j1, b);
    bfly_compute<R>(tw, half, W, ns, k, a);
    if (two) bfly_compute<R>(tw, half, W, ns, k1, b);
    bfly_store<R>(out, ns, j, k, a);
    if (two) bfly_store<R>(out, ns, j1, k1, b);
  }
}

__host__ __device__ inline void pass(int R, const cplx *in, cplx *out, const cplx *tw, int half, int W, int ns, int tid,
                                     int threads) {
  switch (R) {
    case 2: run_pass<2>(in, out, tw, half, W, ns, tid, threads); break;
    case 3: run_pass<3>(in, out, tw, half, W, ns, tid, threads); break;
    case 4: run_pass<4>(in, out, tw, half, W, ns, tid, threads); break;
    default: run_pass<5>(in, out, tw, half, W, ns, tid, threads); break;
  }
}

// |A(k)|^2 and |B(k)|^2, times 4, of the two real rows packed as z = a + i b; zk = Z(k), zm = Z((W - k) mod W)
__host__ __device__ inline void unpack_power(cplx zk, cplx zm, double &pa, double &pb) {
  const double sr = zk.re + zm.re, dr = zk.re - zm.re, si = zk.im + zm.im, di = zk.im - zm.im;
  pa = sr * sr + di * di;
  pb = si * si + dr * dr;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// buf[0] -> ... -> buf[plan.n & 1]; the caller has synchronised after filling buf[0]; ends with a barrier
__device__ __forceinline__ const cplx *transform(cplx (*buf)[kMaxW], const cplx *tw, int half, const Plan &plan, int W) {
  int ns = 1, cur = 0;
  for (int p = 0; p < plan.n; ++p) {
    const int R = plan.radix[p];
    pass(R, buf[cur], buf[cur ^ 1], tw, half, W, ns, threadIdx.x, kThreads);
    __syncthreads();
    ns *= R;
    cur ^= 1;
  }
  return buf[cur];
}

// x_hat / x: [C][H][W].  vec: both base pointers are 16-byte aligned and W % 4 == 0 (every row then starts on 16 bytes).
// kLdsTw: the twiddles are read from an LDS copy of the table's first `half` entries (an even W: W / 2 of them, an odd W
// <= kMaxW / 2: all W), else from the caller's table (half = W).
// slab: [C * bands][3 K + 1] - the band's partial spectra of x, x_hat and d, then its count of non-finite pairs.
template <bool kLdsTw>
__global__ __launch_bounds__(kThreads) void spectrum_partials_kernel(const float *__restrict__ xh, const float *__restrict__ x,
                                                                     int H, int W, int bands,
                                                                     const float *__restrict__ lat_w,
                                                                     const cplx *__restrict__ tw, int half, Plan plan,
                                                                     int vec, double *__restrict__ slab) {
  __shared__ cplx buf[2][kMaxW];
  __shared__ cplx tw_s[kLdsTw ? kMaxW / 2 : 1];
  __shared__ double w_s[kBandRows];
  __shared__ double nf_s[kThreads / 64];
  const int c = blockIdx.x / bands, b = blockIdx.x - c * bands;
  const int r0 = b * kBandRows, nr = min(H, r0 + kBandRows) - r0;   // 1 <= nr <= kBandRows
  const int tid = threadIdx.x;
  const int K = W / 2 + 1;
  for (int r = tid; r < nr; r += kThreads) w_s[r] = lat_w ? (double)lat_w[r0 + r] : 1.0;
  if (kLdsTw)
    for (int i = tid; i < half; i += kThreads) tw_s[i] = tw[i];     // half <= kMaxW / 2 (the launcher's choice)

  const size_t base = ((size_t)c * H + r0) * W;   // the band's first element
  const int W4 = W / 4;
  float4 ph[kVec], pt[kVec];                      // the next row's values (vec)
  auto fetch = [&](int r) {
    const float4 *__restrict__ h4 = reinterpret_cast<const float4 *>(xh + base + (size_t)r * W);
    const float4 *__restrict__ t4 = reinterpret_cast<const float4 *>(x + base + (size_t)r * W);
#pragma unroll
    for (int u = 0; u < kVec; ++u) {
      const int q = tid + u * kThreads;
      if (q < W4) {
        ph[u] = h4[q];
        pt[u] = t4[q];
      }
    }
  };
  unsigned nf = 0;
  // (x, x_hat) of one point into the packed row; returns d.  (Bit tests, as in the error metric: the count must not
  // depend on how the compiler treats NaN; a non-finite pair enters as zeros, its channel is flagged by the count.)
  auto stage = [&](float h, float t, int w) {
    const bool ok = finite_bits(h) && finite_bits(t);
    nf += ok ? 0u : 1u;
    h = ok ? h : 0.f;
    t = ok ? t : 0.f;
    buf[0][w] = {(double)t, (double)h};
    return h - t;
  };
  // the thread's points of a row: 4 (tid + 256 u) + e (vec) or tid + 256 i; their d values of the two rows of a pair
  float d[2][kElems];

  double acc[3][kBins];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < kBins; ++i) acc[s][i] = 0.0;
  // spectra sa (real part of the packed rows, weight la) and sb (imaginary part, weight lb) += weight * 4 |F(k)|^2
  auto accumulate = [&](const cplx *z, int sa, double la, int sb, double lb) {
#pragma unroll
    for (int i = 0; i < kBins; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) {
        double pa, pb;
        unpack_power(z[k], z[k ? W - k : 0], pa, pb);
#pragma unroll
        for (int s = 0; s < 3; ++s) {   // (static register indices)
          if (s == sa) acc[s][i] += la * pa;
          if (s == sb) acc[s][i] += lb * pb;
        }
      }
    }
  };
  auto fft = [&]() { return kLdsTw ? transform(buf, tw_s, half, plan, W) : transform(buf, tw, half, plan, W); };

  if (vec) fetch(0);
  for (int r = 0; r < nr; r += 2) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {   // (unrolled: d[t] stays in registers)
      const int row = r + t;
      if (row < nr) {
        if (vec) {
#pragma unroll
          for (int u = 0; u < kVec; ++u) {
            const int q = tid + u * kThreads;
            if (q < W4) {
              d[t][4 * u] = stage(ph[u].x, pt[u].x, 4 * q);
              d[t][4 * u + 1] = stage(ph[u].y, pt[u].y, 4 * q + 1);
              d[t][4 * u + 2] = stage(ph[u].z, pt[u].z, 4 * q + 2);
              d[t][4 * u + 3] = stage(ph[u].w, pt[u].w, 4 * q + 3);
            }
          }
          if (row + 1 < nr) fetch(row + 1);
        } else {
          const size_t g = base + (size_t)row * W;
#pragma unroll
          for (int i = 0; i < kScalar; ++i) {
            const int w = tid + i * kThreads;
            if (w < W) d[t][i] = stage(xh[g + w], x[g + w], w);
          }
        }
        __syncthreads();
        const cplx *z = fft();
        accumulate(z, 0, w_s[row], 1, w_s[row]);
        __syncthreads();
      } else {
#pragma unroll
        for (int e = 0; e < kElems; ++e) d[t][e] = 0.f;   // the band's odd last row has no partner
      }
    }
    if (vec) {
#pragma unroll
      for (int u = 0; u < kVec; ++u) {
        const int q = tid + u * kThreads;
        if (q < W4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) buf[0][4 * q + e] = {(double)d[0][4 * u + e], (double)d[1][4 * u + e]};
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < kScalar; ++i) {
        const int w = tid + i * kThreads;
        if (w < W) buf[0][w] = {(double)d[0][i], (double)d[1][i]};
      }
    }
    __syncthreads();
    const cplx *z = fft();
    accumulate(z, 2, w_s[r], 2, r + 1 < nr ? w_s[r + 1] : 0.0);
    __syncthreads();
  }

  double *rec = slab + (size_t)blockIdx.x * (3 * K + 1);
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < kBins; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) rec[s * K + k] = acc[s][i];
    }
  const double n = wave_sum((double)nf);
  if ((tid & 63) == 0) nf_s[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    double s = nf_s[0];
    for (int k = 1; k < kThreads / 64; ++k) s += nf_s[k];
    rec[3 * K] = s;
  }
}

// one thread per (spectrum s, bin k) of channel blockIdx.y: the bands in order, then m_k / (4 H W^2) and the flag
__global__ __launch_bounds__(kThreads) void spectrum_finish_kernel(const double *__restrict__ slab, int C, int W, int bands,
                                                                   double scale, double *__restrict__ out,
                                                                   double *__restrict__ nonfinite) {
  const int K = W / 2 + 1, c = blockIdx.y;
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= 3 * K) return;
  const size_t rec = 3 * (size_t)K + 1;
  const double *p = slab + (size_t)c * bands * rec;
  double sum = 0.0, nf = 0.0;
  for (int b = 0; b < bands; ++b) {
    sum += p[b * rec + idx];
    nf += p[b * rec + 3 * K];
  }
  const int s = idx / K, k = idx - s * K;
  const double mk = (k == 0 || 2 * k == W) ? 1.0 : 2.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  out[((size_t)s * C + c) * K + k] = nf > 0 ? nan : sum * scale * mk;
  if (idx == 0) nonfinite[c] = nf;
}

bool dims_ok(int C, int H, int W, Plan &plan) {
  if (!(C > 0 && H > 0 && W >= 2 && W <= kMaxW && (size_t)H * W <= 0x7fffffffu)) return false;
  if (!make_plan(W, plan)) return false;
  return (size_t)C * ((H + kBandRows - 1) / kBandRows) <= 0x7fffffffu && C <= 65535;   // grid.x of pass 1, grid.y of pass 2
}

}  // namespace

extern "C" {

size_t cra5_zonal_spectrum_slab_bytes(int C, int H, int W) {
  Plan plan;
  if (!dims_ok(C, H, W, plan)) return 0;
  return (size_t)C * ((H + kBandRows - 1) / kBandRows) * (3 * (size_t)(W / 2 + 1) + 1) * sizeof(double);
}

int cra5_zonal_spectrum_f32(const float *x_hat, const float *x, int C, int H, int W, const float *lat_w,
                            const double *twiddle, double *slab, size_t slab_bytes, double *out, double *nonfinite,
                            void *stream) {
  Plan plan;
  if (!x_hat || !x || !twiddle || !slab || !out || !nonfinite || !dims_ok(C, H, W, plan)) return CRA5_ERR_ARG;
  if (slab_bytes < cra5_zonal_spectrum_slab_bytes(C, H, W)) return CRA5_ERR_ARG;
  if ((uintptr_t)x_hat % 4 || (uintptr_t)x % 4 || (uintptr_t)twiddle % 16 || (uintptr_t)slab % 8 || (uintptr_t)out % 8 ||
      (uintptr_t)nonfinite % 8 || (lat_w && (uintptr_t)lat_w % 4))
    return CRA5_ERR_ARG;
  const int bands = (H + kBandRows - 1) / kBandRows;
  const int K = W / 2 + 1;
  const int vec = W % 4 == 0 && ((uintptr_t)x_hat % 16) == 0 && ((uintptr_t)x % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  const cplx *tw = reinterpret_cast<const cplx *>(twiddle);
  if (W % 2 == 0 || W <= kMaxW / 2) {
    hipLaunchKernelGGL(spectrum_partials_kernel<true>, dim3(C * bands), dim3(kThreads), 0, st, x_hat, x, H, W, bands, lat_w,
                       tw, W % 2 == 0 ? W / 2 : W, plan, vec, slab);
  } else {
    hipLaunchKernelGGL(spectrum_partials_kernel<false>, dim3(C * bands), dim3(kThreads), 0, st, x_hat, x, H, W, bands, lat_w,
                       tw, W, plan, vec, slab);
  }
  hipLaunchKernelGGL(spectrum_finish_kernel, dim3((3 * K + kThreads - 1) / kThreads, C), dim3(kThreads), 0, st, slab, C, W,
                     bands, 0.25 / ((double)H * W * W), out, nonfinite);
  return (int)hipGetLastError();
}

}  // extern "C"
