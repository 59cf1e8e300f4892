// Per-grid-point statistics over many frames (cra5_time_accumulate_f32 / cra5_time_finish_f32): one streaming
// read-modify-write pass per frame over flat accumulators of the frame's own shape.
//
// Accumulate: element i of the fp32 frame x is folded into sum[i] / sumsq[i] (fp64) and mn[i] / mx[i] (fp32); the first
// frame STORES (no memset, uninitialised accumulators are fine), later ones update.  Every element belongs to exactly one
// thread, so there is nothing to reduce and nothing to order inside a launch: launches on one stream (or chained by
// events) give sum / sumsq the bits of a sequential float64 loop over the frames.  The kernel is specialised on which
// accumulators are present (a NULL one is neither read nor written: `mean` alone moves 4 + 16 bytes per point, all four
// 4 + 48) and on `first`.  With every base 16-byte aligned a thread moves float4 / double2 (several float4 of x and
// their accumulators in flight), the up to three elements past the last float4 go one by one; any unaligned base takes
// the element-wise form for the whole array.  64-bit element indices (268 x 721 x 1440 doubles pass 2^31 bytes); the
// grid is sized to the chip and strides over the array.
// Finish: mean = sum / count, std = sqrt(max(0, (sumsq - sum * sum / count) / (count - ddof))), fp64, uncontracted.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;   // 256 CUs x 8 resident blocks: the grid strides over anything larger
constexpr int kSum = 1, kSumsq = 2, kMin = 4, kMax = 8;

// (bit test, not isnan: the result must not depend on how the compiler treats NaN)
__device__ __forceinline__ bool nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// np.minimum / np.maximum: NaN if either operand is NaN
__device__ __forceinline__ float min_nan(float a, float v) {
  const float m = v < a ? v : a;
  return nan_bits(a) ? a : (nan_bits(v) ? v : m);
}
__device__ __forceinline__ float max_nan(float a, float v) {
  const float m = v > a ? v : a;
  return nan_bits(a) ? a : (nan_bits(v) ? v : m);
}

template <int MASK, bool FIRST>
__device__ __forceinline__ void fold1(float v, size_t e, double *__restrict__ sum, double *__restrict__ sumsq,
                                      float *__restrict__ mn, float *__restrict__ mx) {
  const double d = (double)v;
  // d * d is exact in fp64 (24 x 24 bits): the update rounds once, contracted to an fma or not
  if (MASK & kSum) sum[e] = FIRST ? d : sum[e] + d;
  if (MASK & kSumsq) sumsq[e] = FIRST ? d * d : sumsq[e] + d * d;
  if (MASK & kMin) mn[e] = FIRST ? v : min_nan(mn[e], v);
  if (MASK & kMax) mx[e] = FIRST ? v : max_nan(mx[e], v);
}

// the accumulators of one float4 of x
template <int MASK>
struct Acc4 {
  double2 s[2], q[2];
  float4 lo, hi;
};

template <int MASK>
__device__ __forceinline__ void load4(Acc4<MASK> &a, size_t qi, const double2 *__restrict__ sum2,
                                      const double2 *__restrict__ sumsq2, const float4 *__restrict__ mn4,
                                      const float4 *__restrict__ mx4) {
  if (MASK & kSum) {
    a.s[0] = sum2[2 * qi];
    a.s[1] = sum2[2 * qi + 1];
  }
  if (MASK & kSumsq) {
    a.q[0] = sumsq2[2 * qi];
    a.q[1] = sumsq2[2 * qi + 1];
  }
  if (MASK & kMin) a.lo = mn4[qi];
  if (MASK & kMax) a.hi = mx4[qi];
}

template <int MASK, bool FIRST>
__device__ __forceinline__ void fold4(const float4 &v, Acc4<MASK> &a, size_t qi, double2 *__restrict__ sum2,
                                      double2 *__restrict__ sumsq2, float4 *__restrict__ mn4, float4 *__restrict__ mx4) {
  const double d0 = (double)v.x, d1 = (double)v.y, d2 = (double)v.z, d3 = (double)v.w;
  if (MASK & kSum) {
    sum2[2 * qi] = FIRST ? make_double2(d0, d1) : make_double2(a.s[0].x + d0, a.s[0].y + d1);
    sum2[2 * qi + 1] = FIRST ? make_double2(d2, d3) : make_double2(a.s[1].x + d2, a.s[1].y + d3);
  }
  if (MASK & kSumsq) {
    sumsq2[2 * qi] = FIRST ? make_double2(d0 * d0, d1 * d1) : make_double2(a.q[0].x + d0 * d0, a.q[0].y + d1 * d1);
    sumsq2[2 * qi + 1] = FIRST ? make_double2(d2 * d2, d3 * d3) : make_double2(a.q[1].x + d2 * d2, a.q[1].y + d3 * d3);
  }
  if (MASK & kMin)
    mn4[qi] = FIRST ? v : make_float4(min_nan(a.lo.x, v.x), min_nan(a.lo.y, v.y), min_nan(a.lo.z, v.z), min_nan(a.lo.w, v.w));
  if (MASK & kMax)
    mx4[qi] = FIRST ? v : make_float4(max_nan(a.hi.x, v.x), max_nan(a.hi.y, v.y), max_nan(a.hi.z, v.z), max_nan(a.hi.w, v.w));
}

// nvec: float4 groups taken by the vector body (0: some base is not 16-byte aligned); elements [4 * nvec, n) one by one
template <int MASK, bool FIRST>
__global__ __launch_bounds__(kThreads) void time_accumulate_kernel(const float *__restrict__ x, size_t n, size_t nvec,
                                                                   double *__restrict__ sum, double *__restrict__ sumsq,
                                                                   float *__restrict__ mn, float *__restrict__ mx) {
  // float4 of x in flight per thread, each with its 0 .. 6 accumulator loads: two with both fp64 sums, else four
  constexpr int U = (MASK & (kSum | kSumsq)) == (kSum | kSumsq) ? 2 : 4;
  const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
  double2 *__restrict__ sum2 = reinterpret_cast<double2 *>(sum);
  double2 *__restrict__ sumsq2 = reinterpret_cast<double2 *>(sumsq);
  float4 *__restrict__ mn4 = reinterpret_cast<float4 *>(mn);
  float4 *__restrict__ mx4 = reinterpret_cast<float4 *>(mx);
  const size_t tid = threadIdx.x;
  const size_t chunk = (size_t)kThreads * U, step = (size_t)gridDim.x * chunk;
  for (size_t base = (size_t)blockIdx.x * chunk; base < nvec; base += step) {
    if (base + chunk <= nvec) {
      float4 v[U];
      Acc4<MASK> a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        v[u] = x4[base + u * kThreads + tid];
        if (!FIRST) load4<MASK>(a[u], base + u * kThreads + tid, sum2, sumsq2, mn4, mx4);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) fold4<MASK, FIRST>(v[u], a[u], base + u * kThreads + tid, sum2, sumsq2, mn4, mx4);
    } else {
      for (size_t qi = base + tid; qi < nvec; qi += kThreads) {
        Acc4<MASK> a;
        const float4 v = x4[qi];
        if (!FIRST) load4<MASK>(a, qi, sum2, sumsq2, mn4, mx4);
        fold4<MASK, FIRST>(v, a, qi, sum2, sumsq2, mn4, mx4);
      }
    }
  }
  const size_t threads = (size_t)gridDim.x * kThreads;
  for (size_t e = 4 * nvec + (size_t)blockIdx.x * kThreads + tid; e < n; e += threads)
    fold1<MASK, FIRST>(x[e], e, sum, sumsq, mn, mx);
}

typedef void (*AccumulateKernel)(const float *, size_t, size_t, double *, double *, float *, float *);

template <int MASK>
constexpr AccumulateKernel pick(bool first) {
  return first ? time_accumulate_kernel<MASK, true> : time_accumulate_kernel<MASK, false>;
}

AccumulateKernel accumulate_kernel(int mask, bool first) {
  switch (mask) {
    case 1: return pick<1>(first);
    case 2: return pick<2>(first);
    case 3: return pick<3>(first);
    case 4: return pick<4>(first);
    case 5: return pick<5>(first);
    case 6: return pick<6>(first);
    case 7: return pick<7>(first);
    case 8: return pick<8>(first);
    case 9: return pick<9>(first);
    case 10: return pick<10>(first);
    case 11: return pick<11>(first);
    case 12: return pick<12>(first);
    case 13: return pick<13>(first);
    case 14: return pick<14>(first);
    case 15: return pick<15>(first);
  }
  return nullptr;
}

int grid_for(size_t work_items) {
  const size_t blocks = (work_items + kThreads - 1) / kThreads;
  return (int)(blocks < 1 ? 1 : (blocks > (size_t)kMaxBlocks ? (size_t)kMaxBlocks : blocks));
}

// every operation rounds on its own, in the written association: product, quotient, difference, quotient
__global__ __launch_bounds__(kThreads) void time_finish_kernel(size_t n, double count, double dof,
                                                               const double *__restrict__ sum,
                                                               const double *__restrict__ sumsq, float *__restrict__ mean,
                                                               float *__restrict__ stdv) {
#pragma clang fp contract(off)
  const size_t threads = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += threads) {
    const double s = sum[e];
    if (mean) mean[e] = (float)(s / count);
    if (stdv) {
      const double p = s * s;
      const double m = p / count;
      const double d = sumsq[e] - m;
      const double var = d / dof;
      stdv[e] = (float)sqrt(var < 0.0 ? 0.0 : var);   // (NaN stays NaN: the comparison is false)
    }
  }
}

}  // namespace

extern "C" {

int cra5_time_accumulate_f32(const float *x, size_t n, int first, double *sum, double *sumsq, float *mn, float *mx,
                             void *stream) {
  const int mask = (sum ? kSum : 0) | (sumsq ? kSumsq : 0) | (mn ? kMin : 0) | (mx ? kMax : 0);
  if (!x || n == 0 || mask == 0) return CRA5_ERR_ARG;
  if ((uintptr_t)x % 4 || (uintptr_t)mn % 4 || (uintptr_t)mx % 4 || (uintptr_t)sum % 8 || (uintptr_t)sumsq % 8)
    return CRA5_ERR_ARG;
  const bool vec = !((uintptr_t)x % 16 || (uintptr_t)sum % 16 || (uintptr_t)sumsq % 16 || (uintptr_t)mn % 16 ||
                     (uintptr_t)mx % 16);
  const size_t nvec = vec ? n / 4 : 0;
  // one thread per float4 of a block's chunk (the kernel strides by whole chunks), or per element without the vector body
  const int U = (mask & (kSum | kSumsq)) == (kSum | kSumsq) ? 2 : 4;
  const int grid = nvec ? grid_for((nvec + U - 1) / U) : grid_for(n);
  hipLaunchKernelGGL(accumulate_kernel(mask, first != 0), dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x, n, nvec,
                     sum, sumsq, mn, mx);
  return (int)hipGetLastError();
}

int cra5_time_finish_f32(size_t n, long long count, int ddof, const double *sum, const double *sumsq, float *mean,
                         float *stdv, void *stream) {
  if (n == 0 || !sum || (!mean && !stdv) || (stdv && !sumsq)) return CRA5_ERR_ARG;
  if (count < 1 || ddof < 0 || count - ddof < 1) return CRA5_ERR_ARG;
  if ((uintptr_t)sum % 8 || (uintptr_t)sumsq % 8 || (uintptr_t)mean % 4 || (uintptr_t)stdv % 4) return CRA5_ERR_ARG;
  hipLaunchKernelGGL(time_finish_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, n, (double)count,
                     (double)(count - ddof), sum, sumsq, mean, stdv);
  return (int)hipGetLastError();
}

}  // extern "C"
