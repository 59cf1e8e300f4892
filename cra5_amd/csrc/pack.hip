// Packed int16 output of a frame ("Packed int16 output"): cra5_pack_range_f32 measures every channel
// and derives its scale / offset on the device, cra5_pack_i16_f32 turns the frame into int16 codes with them.
//
// Range, pass 1 (pack_range_partials_kernel): one block per (channel, band of kBandElems elements of the flat plane).
// Every thread keeps the min and the max of its FINITE elements and the count of the others; min / max run on an
// order-preserving integer key of the fp32 bit pattern, so they are exact whatever the denormal mode and never see a NaN.
// The block reduces with the fixed 64-lane butterfly, then across its waves through LDS, and writes ONE record to the
// caller's slab [C][bands] with plain stores: no memset, no atomics.  Pass 2 (pack_range_finish_kernel): one wave per
// channel reduces the bands in a fixed order and computes scale / offset (rule 3) - no host round trip between measuring
// and packing.  Fixed reduction order: the table is bit-identical from run to run.
//
// Pack (pack_i16_kernel): one block per (channel, chunk).  The chunk's codes are cut where the DESTINATION is 8-byte
// aligned: four codes per 8-byte store, their four floats one 16-byte load (of 4-byte alignment when source and destination
// differ in phase); the up to three codes in front of and behind a plane's aligned part are written one by one.
//
// Unpack (unpack_i16_kernel; DESIGN.md section 4, "Packed int16 input"): the way in, cra5_unpack_i16_f32.  The same grid,
// cut where the fp32 DESTINATION is 16-byte aligned: one 16-byte store per four values, their four codes one 8-byte load
// (of 2-byte alignment when the phases differ), bytes swapped in registers when the codes come in the other byte order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBandElems = kThreads * 96;   // range pass: ~96 elements per thread per band
constexpr int kChunkGroups = kThreads * 16; // pack pass: 16 groups of four codes per thread per chunk

struct Rec {
  unsigned mn, mx, nf, pad;   // keys of the finite min / max (0xffffffff / 0: none seen), count of non-finite elements
};

__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }

// a < b as floats  <=>  key(a) < key(b) as unsigned (-0 sorts below +0); no finite value has the key 0 or 0xffffffff
__device__ __forceinline__ unsigned key_of(unsigned u) { return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
// (the two empty keys come back as NaN patterns: 0xffffffff -> 0x7fffffff, 0 -> 0xffffffff)
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

struct Acc {
  unsigned mn = 0xffffffffu, mx = 0u, nf = 0u;
};

__device__ __forceinline__ void add(Acc &a, float v) {
  const unsigned u = __float_as_uint(v);
  const bool ok = finite_bits(u);
  const unsigned k = key_of(u);
  a.nf += ok ? 0u : 1u;
  a.mn = min(a.mn, ok ? k : 0xffffffffu);
  a.mx = max(a.mx, ok ? k : 0u);
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, off, 64));
  return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, 64));
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
  return v;
}

// x: [C][plane].  xph: (address of x / 4) % 4 - element e is 16-byte aligned when (e + xph) % 4 == 0.
__global__ __launch_bounds__(kThreads) void pack_range_partials_kernel(const float *__restrict__ x, unsigned plane,
                                                                       int bands, unsigned xph, Rec *__restrict__ slab) {
  __shared__ Rec red[kThreads / 64];
  const int c = blockIdx.x / bands, b = blockIdx.x - c * bands;
  const int tid = threadIdx.x;
  const size_t cbase = (size_t)c * plane;
  const size_t g0 = cbase + (size_t)b * kBandElems;
  const size_t g1 = min(cbase + plane, g0 + kBandElems);
  // [g0, a0) and [a1, g1) element by element, [a0, a1) as float4
  const size_t a0 = min(((g0 + xph + 3) & ~(size_t)3) - xph, g1);
  const size_t a1 = a0 < g1 ? ((g1 + xph) & ~(size_t)3) - xph : a0;
  Acc acc;
  for (size_t e = g0 + tid; e < a0; e += kThreads) add(acc, x[e]);
  for (size_t e = a1 + tid; e < g1; e += kThreads) add(acc, x[e]);

  const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x - (ptrdiff_t)xph);   // (16-byte aligned; [0] unread)
  const size_t q1 = (a1 + xph) / 4;
  size_t q = (a0 + xph) / 4 + tid;
  auto body = [&](const float4 &v) {
    add(acc, v.x);
    add(acc, v.y);
    add(acc, v.z);
    add(acc, v.w);
  };
  // eight float4 in flight per thread
  for (; q + 7 * kThreads < q1; q += 8 * kThreads) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = x4[q + u * kThreads];
#pragma unroll
    for (int u = 0; u < 8; ++u) body(v[u]);
  }
  for (; q < q1; q += kThreads) body(x4[q]);

  const unsigned mn = wave_min(acc.mn), mx = wave_max(acc.mx);
  const unsigned nf = (unsigned)wave_sum((unsigned long long)acc.nf);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) red[wave] = Rec{mn, mx, nf, 0u};
  __syncthreads();
  if (tid == 0) {
    Rec r = red[0];
    for (int k = 1; k < kThreads / 64; ++k) {
      r.mn = min(r.mn, red[k].mn);
      r.mx = max(r.mx, red[k].mx);
      r.nf += red[k].nf;
    }
    slab[blockIdx.x] = r;
  }
}

// one wave per channel: lane l reduces bands l, l + 64, ... in order, then the fixed butterfly; lane 0 applies rule 3
__global__ __launch_bounds__(64) void pack_range_finish_kernel(const Rec *__restrict__ slab, int bands,
                                                               const double *__restrict__ fixed,
                                                               double *__restrict__ out) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const Rec *p = slab + (size_t)c * bands;
  unsigned mn = 0xffffffffu, mx = 0u;
  unsigned long long nf = 0;
  for (int b = lane; b < bands; b += 64) {
    mn = min(mn, p[b].mn);
    mx = max(mx, p[b].mx);
    nf += p[b].nf;
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  nf = wave_sum(nf);
  if (lane) return;
  const bool any = mn != 0xffffffffu;
  const double vmin = (double)value_of(mn), vmax = (double)value_of(mx);   // NaN without a finite element
  double lo = vmin, hi = vmax;
  bool have = any;
  if (fixed) {
    const double flo = fixed[2 * c], fhi = fixed[2 * c + 1];
    if (flo == flo) {   // a NaN lo: this channel takes its own range
      lo = flo;
      hi = fhi;
      have = true;
    }
  }
  double scale = 1.0, offset = 0.0;
  if (have) {
    if (lo == hi) {
      offset = lo;
    } else {
      scale = (hi - lo) / 65534.0;
      offset = (lo + hi) * 0.5;
    }
  }
  double *o = out + (size_t)c * CRA5_PACK_FIELDS;
  o[CRA5_PACK_VMIN] = vmin;
  o[CRA5_PACK_VMAX] = vmax;
  o[CRA5_PACK_NONFINITE] = (double)nf;
  o[CRA5_PACK_SCALE] = scale;
  o[CRA5_PACK_OFFSET] = offset;
}

// rule 4: true float64 subtraction and division, ties to even, the clamp in float64 before the conversion
__device__ __forceinline__ unsigned code_of(float v, double scale, double offset) {
  const double r = fmin(fmax(rint(((double)v - offset) / scale), -32767.0), 32767.0);
  const int q = finite_bits(__float_as_uint(v)) ? (int)r : -32768;
  return (unsigned)q & 0xffffu;
}

struct __attribute__((aligned(4))) Float4A4 {   // four floats at 4-byte alignment: one 16-byte load
  float x, y, z, w;
};

// x: [C][plane] -> q: [C][plane] int16.  qph: (address of q / 2) % 4 - code e is 8-byte aligned when (e + qph) % 4 == 0.
__global__ __launch_bounds__(kThreads) void pack_i16_kernel(const float *__restrict__ x, unsigned plane, int chunks,
                                                            unsigned qph, const double *__restrict__ table,
                                                            unsigned short *__restrict__ q) {
  const int c = blockIdx.x / chunks, b = blockIdx.x - c * chunks;
  const int tid = threadIdx.x;
  const double scale = table[(size_t)c * CRA5_PACK_FIELDS + CRA5_PACK_SCALE];
  const double offset = table[(size_t)c * CRA5_PACK_FIELDS + CRA5_PACK_OFFSET];
  const size_t g0 = (size_t)c * plane, g1 = g0 + plane;
  const size_t a0 = min(((g0 + qph + 3) & ~(size_t)3) - qph, g1);
  const size_t a1 = a0 < g1 ? ((g1 + qph) & ~(size_t)3) - qph : a0;
  if (b == 0) {
    // the plane's head [g0, a0) and tail [a1, g1): at most three codes each
    if (g0 + tid < a0) q[g0 + tid] = (unsigned short)code_of(x[g0 + tid], scale, offset);
    if (tid >= 64 && a1 + (tid - 64) < g1) q[a1 + (tid - 64)] = (unsigned short)code_of(x[a1 + (tid - 64)], scale, offset);
  }
  const size_t n_groups = (a1 - a0) / 4;
  const size_t j1 = min(n_groups, (size_t)(b + 1) * kChunkGroups);
  for (size_t j = (size_t)b * kChunkGroups + tid; j < j1; j += kThreads) {
    const size_t e = a0 + 4 * j;
    const Float4A4 v = *reinterpret_cast<const Float4A4 *>(x + e);
    uint2 w;
    w.x = code_of(v.x, scale, offset) | (code_of(v.y, scale, offset) << 16);
    w.y = code_of(v.z, scale, offset) | (code_of(v.w, scale, offset) << 16);
    *reinterpret_cast<uint2 *>(q + e) = w;
  }
}

// "Packed int16 input": two float64 roundings (a multiply, then an add - never one fused operation, whatever the build's
// contraction setting), one rounding to fp32, one fp32 multiply; the code FILL[c] gives the quiet NaN (a NaN FILL equals
// no code)
__device__ __forceinline__ float value_of_code(int q, double scale, double offset, double fill, float mul) {
#pragma clang fp contract(off)
  const double dq = (double)q;
  const double p = dq * scale;
  const double d = p + offset;
  const float v = __double2float_rn(d) * mul;
  return dq == fill ? __uint_as_float(0x7fc00000u) : v;
}

// the two codes of a 32-bit word, low half first; swapped: each half's bytes change places first
__device__ __forceinline__ unsigned swap_halves(unsigned w, bool swapped) {
  return swapped ? ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu) : w;
}
__device__ __forceinline__ int code_lo(unsigned w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int code_hi(unsigned w) { return (int)w >> 16; }

struct __attribute__((aligned(2))) Word2A2 {   // four codes at 2-byte alignment: one 8-byte load
  unsigned short h[4];
};

// q: [C][plane] int16 -> x: [C][plane].  xph: (address of x / 4) % 4 - value e is 16-byte aligned when (e + xph) % 4 == 0.
__global__ __launch_bounds__(kThreads) void unpack_i16_kernel(const unsigned short *__restrict__ q, unsigned plane,
                                                              int chunks, unsigned xph, const double *__restrict__ table,
                                                              unsigned flags, float *__restrict__ x) {
  const int c = blockIdx.x / chunks, b = blockIdx.x - c * chunks;
  const int tid = threadIdx.x;
  const bool swapped = (flags & CRA5_UNPACK_SWAPPED) != 0;
  const double *t = table + (size_t)c * CRA5_UNPACK_FIELDS;
  const double scale = t[0], offset = t[1], fill = t[2];
  const float mul = (float)t[3];
  const size_t g0 = (size_t)c * plane, g1 = g0 + plane;
  const size_t a0 = min(((g0 + xph + 3) & ~(size_t)3) - xph, g1);
  const size_t a1 = a0 < g1 ? ((g1 + xph) & ~(size_t)3) - xph : a0;
  auto one = [&](size_t e) { x[e] = value_of_code(code_lo(swap_halves(q[e], swapped)), scale, offset, fill, mul); };
  if (b == 0) {
    // the plane's head [g0, a0) and tail [a1, g1): at most three values each
    if (g0 + tid < a0) one(g0 + tid);
    if (tid >= 64 && a1 + (tid - 64) < g1) one(a1 + (tid - 64));
  }
  const size_t n_groups = (a1 - a0) / 4;
  const size_t j1 = min(n_groups, (size_t)(b + 1) * kChunkGroups);
  auto group = [&](size_t e, const Word2A2 &v) {
    const unsigned w0 = swap_halves(v.h[0] | ((unsigned)v.h[1] << 16), swapped);
    const unsigned w1 = swap_halves(v.h[2] | ((unsigned)v.h[3] << 16), swapped);
    float4 o;
    o.x = value_of_code(code_lo(w0), scale, offset, fill, mul);
    o.y = value_of_code(code_hi(w0), scale, offset, fill, mul);
    o.z = value_of_code(code_lo(w1), scale, offset, fill, mul);
    o.w = value_of_code(code_hi(w1), scale, offset, fill, mul);
    *reinterpret_cast<float4 *>(x + e) = o;
  };
  size_t j = (size_t)b * kChunkGroups + tid;
  // four loads in flight per thread
  for (; j + 3 * kThreads < j1; j += 4 * kThreads) {
    Word2A2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const Word2A2 *>(q + a0 + 4 * (j + u * kThreads));
#pragma unroll
    for (int u = 0; u < 4; ++u) group(a0 + 4 * (j + u * kThreads), v[u]);
  }
#pragma unroll 1
  for (; j < j1; j += kThreads) {
    const Word2A2 v = *reinterpret_cast<const Word2A2 *>(q + a0 + 4 * j);
    group(a0 + 4 * j, v);
  }
}

bool dims_ok(int C, size_t plane) { return C > 0 && plane > 0 && plane <= 0x7fffffffu; }

int bands_of(size_t plane) { return (int)((plane + kBandElems - 1) / kBandElems); }

}  // namespace

extern "C" {

size_t cra5_pack_range_slab_bytes(int C, size_t plane) {
  if (!dims_ok(C, plane)) return 0;
  return (size_t)C * bands_of(plane) * sizeof(Rec);
}

int cra5_pack_range_f32(const float *x, int C, size_t plane, const double *fixed, void *slab, size_t slab_bytes,
                        double *out, void *stream) {
  if (!x || !slab || !out || !dims_ok(C, plane)) return CRA5_ERR_ARG;
  if (slab_bytes < cra5_pack_range_slab_bytes(C, plane)) return CRA5_ERR_ARG;
  if ((uintptr_t)x % 4 || (uintptr_t)slab % 16 || (uintptr_t)out % 8 || (uintptr_t)fixed % 8) return CRA5_ERR_ARG;
  const int bands = bands_of(plane);
  if ((size_t)C * bands > 0x7fffffffu) return CRA5_ERR_ARG;
  const unsigned xph = (unsigned)(((uintptr_t)x / 4) % 4);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pack_range_partials_kernel, dim3(C * bands), dim3(kThreads), 0, st, x, (unsigned)plane, bands, xph,
                     (Rec *)slab);
  hipLaunchKernelGGL(pack_range_finish_kernel, dim3(C), dim3(64), 0, st, (const Rec *)slab, bands, fixed, out);
  return (int)hipGetLastError();
}

int cra5_pack_i16_f32(const float *x, int C, size_t plane, const double *table, int16_t *q, void *stream) {
  if (!x || !table || !q || !dims_ok(C, plane)) return CRA5_ERR_ARG;
  if ((uintptr_t)x % 4 || (uintptr_t)q % 2 || (uintptr_t)table % 8) return CRA5_ERR_ARG;
  // (the aligned part of a plane holds at most plane / 4 groups)
  const int chunks = (int)((plane / 4 + kChunkGroups - 1) / kChunkGroups) + (plane < 4 ? 1 : 0);
  if ((size_t)C * chunks > 0x7fffffffu) return CRA5_ERR_ARG;
  const unsigned qph = (unsigned)(((uintptr_t)q / 2) % 4);
  hipLaunchKernelGGL(pack_i16_kernel, dim3(C * chunks), dim3(kThreads), 0, (hipStream_t)stream, x, (unsigned)plane, chunks,
                     qph, table, (unsigned short *)q);
  return (int)hipGetLastError();
}

int cra5_unpack_i16_f32(const int16_t *q, int C, size_t plane, const double *table, unsigned flags, float *x,
                        void *stream) {
  if (!q || !table || !x || !dims_ok(C, plane)) return CRA5_ERR_ARG;
  if ((uintptr_t)q % 2 || (uintptr_t)x % 4 || (uintptr_t)table % 8 || (flags & ~CRA5_UNPACK_SWAPPED)) return CRA5_ERR_ARG;
  const int chunks = (int)((plane / 4 + kChunkGroups - 1) / kChunkGroups) + (plane < 4 ? 1 : 0);
  if ((size_t)C * chunks > 0x7fffffffu) return CRA5_ERR_ARG;
  const unsigned xph = (unsigned)(((uintptr_t)x / 4) % 4);
  hipLaunchKernelGGL(unpack_i16_kernel, dim3(C * chunks), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned short *)q, (unsigned)plane, chunks, xph, table, flags, x);
  return (int)hipGetLastError();
}

}  // extern "C"
