// Per-channel reconstruction error of a frame: one streaming pass over x_hat and x (cra5_recon_error_f32).
//
// Pass 1 (recon_partials_kernel): one block per (channel, band of rows).  Every thread accumulates, in fp32, d, d^2,
// L(h) d^2 and |d| over ~100 elements (d = x_hat - x), beside the max of |d| and the count of non-finite pairs (those are
// left out of the sums); the block reduces in fp64 across the wave and then across the waves through LDS, always in the
// same order, and writes ONE record to the caller's slab [C][bands][CRA5_RECON_FIELDS].  Plain stores: no memset, no
// atomics.  Pass 2 (recon_finish_kernel): one wave per channel sums its bands in a fixed order.  Both passes have a fixed
// reduction order, so the result is bit-identical from run to run and whatever else runs beside it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBandElems = kThreads * 96;   // ~96 elements per thread per band
constexpr int kMaxBandRows = 1024;          // the band's latitude weights are staged in LDS

__host__ __device__ inline int band_rows(int W) {
  int r = kBandElems / W;
  return r < 1 ? 1 : (r > kMaxBandRows ? kMaxBandRows : r);
}

struct Acc {
  float s1 = 0.f, s2 = 0.f, sw = 0.f, sa = 0.f, mx = 0.f;
  unsigned nf = 0;
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void add(Acc &a, float h, float t, float w) {
  // (bit tests, not isfinite: the count must not depend on how the compiler treats NaN)
  const bool ok = finite_bits(h) && finite_bits(t);
  const float d = ok ? h - t : 0.f;
  const float dd = d * d;
  const float ad = fabsf(d);
  a.nf += ok ? 0u : 1u;
  a.s1 += d;
  a.s2 += dd;
  a.sw = fmaf(w, dd, a.sw);
  a.sa += ad;
  a.mx = fmaxf(a.mx, ad);   // (ad is finite or +inf here, never NaN)
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// x_hat / x: [C][H][W].  vec: both base pointers are 16-byte aligned and W >= 4 (a float4 then spans at most two rows).
__global__ __launch_bounds__(kThreads) void recon_partials_kernel(const float *__restrict__ xh, const float *__restrict__ x,
                                                                  int H, int W, int rows, int bands,
                                                                  const float *__restrict__ lat_w, int vec,
                                                                  double *__restrict__ slab) {
  __shared__ float w_s[kMaxBandRows];
  __shared__ double red[kThreads / 64][CRA5_RECON_FIELDS];
  const int c = blockIdx.x / bands, b = blockIdx.x - c * bands;
  const int r0 = b * rows, r1 = min(H, r0 + rows);
  const int tid = threadIdx.x;
  for (int r = tid; r < r1 - r0; r += kThreads) w_s[r] = lat_w ? lat_w[r0 + r] : 1.f;
  __syncthreads();

  const size_t cbase = (size_t)c * H * W;
  const size_t g0 = cbase + (size_t)r0 * W, g1 = cbase + (size_t)r1 * W;
  // [g0, a0) and [a1, g1) element by element, [a0, a1) as float4 (empty without vec)
  size_t a0 = g1, a1 = g1;
  if (vec) {
    a0 = min((g0 + 3) & ~(size_t)3, g1);
    a1 = max(g1 & ~(size_t)3, a0);
  }
  Acc acc;
  for (size_t e = g0 + tid; e < a0; e += kThreads) add(acc, xh[e], x[e], w_s[(unsigned)(e - cbase) / (unsigned)W - r0]);
  for (size_t e = a1 + tid; e < g1; e += kThreads) add(acc, xh[e], x[e], w_s[(unsigned)(e - cbase) / (unsigned)W - r0]);

  const float4 *__restrict__ xh4 = reinterpret_cast<const float4 *>(xh);
  const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
  const size_t q1 = a1 / 4;
  size_t q = a0 / 4 + tid;
  auto body = [&](const float4 &h, const float4 &t, size_t qq) {
    const unsigned l = (unsigned)(4 * qq - cbase);   // element index inside the channel plane
    const unsigned row = l / (unsigned)W;
    const unsigned rem = l - row * (unsigned)W;
    const float w0 = w_s[row - r0];
    // a float4 crosses into the next row only when W % 4 != 0; that row is then inside the band (the float4 is)
    const float w1 = rem + 3 >= (unsigned)W ? w_s[row + 1 - r0] : w0;
    add(acc, h.x, t.x, w0);
    add(acc, h.y, t.y, rem + 1 >= (unsigned)W ? w1 : w0);
    add(acc, h.z, t.z, rem + 2 >= (unsigned)W ? w1 : w0);
    add(acc, h.w, t.w, w1);
  };
  // four float4 of each input in flight per thread
  for (; q + 3 * kThreads < q1; q += 4 * kThreads) {
    float4 h[4], t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      h[u] = xh4[q + u * kThreads];
      t[u] = x4[q + u * kThreads];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) body(h[u], t[u], q + u * kThreads);
  }
  for (; q < q1; q += kThreads) body(xh4[q], x4[q], q);

  double v[CRA5_RECON_FIELDS] = {wave_sum(acc.s1), wave_sum(acc.s2), wave_sum(acc.sw), wave_sum(acc.sa),
                                 wave_max(acc.mx), wave_sum((double)acc.nf)};
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int f = 0; f < CRA5_RECON_FIELDS; ++f) red[wave][f] = v[f];
  }
  __syncthreads();
  if (tid < CRA5_RECON_FIELDS) {
    double s = red[0][tid];
    for (int k = 1; k < kThreads / 64; ++k) s = tid == CRA5_RECON_MAX_ABS ? fmax(s, red[k][tid]) : s + red[k][tid];
    slab[(size_t)blockIdx.x * CRA5_RECON_FIELDS + tid] = s;
  }
}

// one wave per channel: lane l sums bands l, l + 64, ... in order, then the fixed butterfly
__global__ __launch_bounds__(64) void recon_finish_kernel(const double *__restrict__ slab, int bands, double inv_n,
                                                          double *__restrict__ out) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const double *p = slab + (size_t)c * bands * CRA5_RECON_FIELDS;
  double s1 = 0, s2 = 0, sw = 0, sa = 0, mx = 0, nf = 0;
  for (int b = lane; b < bands; b += 64) {
    const double *r = p + (size_t)b * CRA5_RECON_FIELDS;
    s1 += r[CRA5_RECON_BIAS];
    s2 += r[CRA5_RECON_MSE];
    sw += r[CRA5_RECON_WMSE];
    sa += r[CRA5_RECON_MAE];
    mx = fmax(mx, r[CRA5_RECON_MAX_ABS]);
    nf += r[CRA5_RECON_NONFINITE];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  sw = wave_sum(sw);
  sa = wave_sum(sa);
  mx = wave_max(mx);
  nf = wave_sum(nf);
  if (lane) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double *o = out + (size_t)c * CRA5_RECON_FIELDS;
  o[CRA5_RECON_BIAS] = nf > 0 ? nan : s1 * inv_n;
  o[CRA5_RECON_MSE] = nf > 0 ? nan : s2 * inv_n;
  o[CRA5_RECON_WMSE] = nf > 0 ? nan : sw * inv_n;
  o[CRA5_RECON_MAE] = nf > 0 ? nan : sa * inv_n;
  o[CRA5_RECON_MAX_ABS] = nf > 0 ? nan : mx;
  o[CRA5_RECON_NONFINITE] = nf;
}

bool dims_ok(int C, int H, int W) {
  return C > 0 && H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu;
}

}  // namespace

extern "C" {

size_t cra5_recon_error_slab_bytes(int C, int H, int W) {
  if (!dims_ok(C, H, W)) return 0;
  const int rows = band_rows(W);
  return (size_t)C * ((H + rows - 1) / rows) * CRA5_RECON_FIELDS * sizeof(double);
}

int cra5_recon_error_f32(const float *x_hat, const float *x, int C, int H, int W, const float *lat_w, double *slab,
                         size_t slab_bytes, double *out, void *stream) {
  if (!x_hat || !x || !slab || !out || !dims_ok(C, H, W)) return CRA5_ERR_ARG;
  if (slab_bytes < cra5_recon_error_slab_bytes(C, H, W)) return CRA5_ERR_ARG;
  const int rows = band_rows(W);
  const int bands = (H + rows - 1) / rows;
  if ((size_t)C * bands > 0x7fffffffu) return CRA5_ERR_ARG;
  const int vec = W >= 4 && ((uintptr_t)x_hat % 16) == 0 && ((uintptr_t)x % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(recon_partials_kernel, dim3(C * bands), dim3(kThreads), 0, st, x_hat, x, H, W, rows, bands, lat_w,
                     vec, slab);
  hipLaunchKernelGGL(recon_finish_kernel, dim3(C), dim3(64), 0, st, slab, bands, 1.0 / ((double)H * W), out);
  return (int)hipGetLastError();
}

}  // extern "C"
