// Exact per-channel quantiles of truth, reconstruction and |error| of a frame pair (cra5_frame_quantiles_f32; DESIGN.md
// section 4, "Quantiles"): an MSD radix select over order-preserving uint32 keys, four digit passes of 8 bits.
//
// Every digit pass (quantile_count_kernel) streams x_hat and x once, with the access pattern of metrics.hip: one block per
// (channel, band of rows), the band's integer row weights staged in LDS, float4 loads where both bases are 16-byte aligned
// and W >= 4, four loads of each input in flight per thread.  Per element it forms the three keys (x, x_hat, |x_hat - x|),
// matches each key's already decided digits against the channel's live prefixes (at most NS = Q rounded up to a power of
// two; the quantiles that share a prefix share one slot) and adds the row weight to the LDS histogram bin [field][slot][
// digit].  The block then adds its non-zero bins to the global histograms with 64-bit integer atomics.
// quantile_select_kernel (one wave per (channel, field)) picks, for each of the Q targets, the digit whose cumulative
// weight first reaches the remaining target, extends the prefix, de-duplicates the prefixes for the next pass and clears
// the bins it read.  After the fourth pass the prefix is the key of the answer.
//
// Contention (the first digit of a smooth field is one bin for the whole channel): PER-THREAD RUN ACCUMULATION.  A thread
// keeps, per field, the bin of its last element and the weight summed for it in registers, and touches LDS only when the
// bin changes and once at the end of its band; a thread's elements are four neighbours in a row and then the same columns
// 1.4 or 2.8 rows further on, so on smooth fields the first two digits cost a handful of LDS atomics per thread, not one per
// element.  The later digits are close to uniform: runs have length one there, which is one atomic per element that
// still matches a live prefix - and few elements do.
//
// Counters: LDS and global bins are 64-bit.  A block's band has < 2^31 elements of weight <= 2^20, so no bin can pass
// 2^51; a channel's total is W * sum w_h < 2^53.  All counting is in unsigned integers: any order of the atomics gives the
// same bits, so the result is identical from run to run and whatever else runs beside it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

typedef unsigned long long u64;

constexpr int kBandElems = 24576;           // the band of metrics.hip: 17 rows of 1440
// threads per block (48 elements per thread); the 16-slot histograms fill 96 KB of LDS, so only one such block fits a CU:
// it gets twice the threads (24 elements each)
__host__ __device__ constexpr int threads_for(int NS) { return NS > 8 ? 1024 : 512; }
constexpr int kMaxBandRows = 1024;          // the band's row weights are staged in LDS
constexpr int kMaxQ = CRA5_QUANTILE_MAX_Q;
constexpr unsigned kNoPrefix = 0xffffffffu;   // never equals key >> s for s >= 8

__host__ __device__ inline int band_rows(int W) {
  int r = kBandElems / W;
  return r < 1 ? 1 : (r > kMaxBandRows ? kMaxBandRows : r);
}

inline int slots_for(int Q) { return Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : Q <= 8 ? 8 : 16; }

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// fp32 bits -> uint32 whose unsigned order is the order of the values; -0 and +0 share a key
__device__ __forceinline__ unsigned key_of(float v) {
  unsigned u = __float_as_uint(v);
  u = u == 0x80000000u ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// the workspace: the global histograms, then the per-(channel, field) selection state
struct Ws {
  u64 *hist;        // [C][3][NS][256]
  u64 *rem;         // [C][3][kMaxQ]   remaining target of quantile q inside its prefix
  unsigned *prefix; // [C][3][kMaxQ]   decided digits of quantile q
  unsigned *live;   // [C][3][kMaxQ]   distinct prefixes, padded with kNoPrefix
  unsigned *slot;   // [C][3][kMaxQ]   quantile q -> index into live
  unsigned *nlive;  // [C][3]
  unsigned *nonfinite;  // [C]
};

size_t ws_layout(int C, int NS, void *base, Ws *w) {
  const size_t cf = (size_t)C * 3;
  size_t off = 0;
  char *p = (char *)base;
  auto take = [&](size_t bytes) {
    char *r = p + off;
    off += (bytes + 7) & ~(size_t)7;
    return r;
  };
  u64 *hist = (u64 *)take(cf * NS * 256 * sizeof(u64));
  u64 *rem = (u64 *)take(cf * kMaxQ * sizeof(u64));
  unsigned *prefix = (unsigned *)take(cf * kMaxQ * sizeof(unsigned));
  unsigned *live = (unsigned *)take(cf * kMaxQ * sizeof(unsigned));
  unsigned *slot = (unsigned *)take(cf * kMaxQ * sizeof(unsigned));
  unsigned *nlive = (unsigned *)take(cf * sizeof(unsigned));
  unsigned *nonfinite = (unsigned *)take((size_t)C * sizeof(unsigned));
  if (w) *w = Ws{hist, rem, prefix, live, slot, nlive, nonfinite};
  return off;
}

__global__ __launch_bounds__(256) void quantile_init_kernel(Ws ws, size_t hist_n, int C, int Q,
                                                            const u64 *__restrict__ targets) {
  const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  for (size_t i = i0; i < hist_n; i += step) ws.hist[i] = 0;
  for (size_t i = i0; i < (size_t)C * 3 * kMaxQ; i += step) {
    const int q = (int)(i % kMaxQ);
    ws.rem[i] = q < Q ? targets[q] : 0;
    ws.prefix[i] = 0;
    ws.live[i] = q == 0 ? 0u : kNoPrefix;
    ws.slot[i] = 0;
  }
  for (size_t i = i0; i < (size_t)C * 3; i += step) ws.nlive[i] = 1;
  for (size_t i = i0; i < (size_t)C; i += step) ws.nonfinite[i] = 0;
}

// One digit pass.  shift: the digit is (key >> shift) & 255, the prefix key >> (shift + 8).  FIRST: no prefix yet, one
// slot, and the pass that counts the non-finite pairs.  gs: slots per (channel, field) of the global histograms.
// vec: both base pointers are 16-byte aligned and W >= 4 (a float4 then spans at most two rows).
template <int NS, bool FIRST>
__global__ __launch_bounds__(threads_for(NS)) void quantile_count_kernel(
    const float *__restrict__ xh, const float *__restrict__ x, int H, int W, int rows, int bands,
    const unsigned *__restrict__ row_w, int vec, int shift, const unsigned *__restrict__ live,
    const unsigned *__restrict__ nlive, int gs, u64 *__restrict__ hist_g, unsigned *__restrict__ nonfinite_g) {
  constexpr int kThreads = threads_for(NS);
  __shared__ u64 hist[3 * NS * 256];
  __shared__ unsigned w_s[kMaxBandRows];
  __shared__ unsigned nf_s;
  const int c = blockIdx.x / bands, b = blockIdx.x - c * bands;
  const int r0 = b * rows, r1 = min(H, r0 + rows);
  const int tid = threadIdx.x;
  // the slots in use (uniform): only they are cleared, matched against and flushed
  int nl[3], nlmax = 1;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    nl[f] = FIRST ? 1 : min((int)nlive[(size_t)c * 3 + f], NS);
    nlmax = max(nlmax, nl[f]);
  }
#pragma unroll
  for (int f = 0; f < 3; ++f)
    for (int i = tid; i < nlmax * 256; i += kThreads) hist[f * NS * 256 + i] = 0;
  for (int r = tid; r < r1 - r0; r += kThreads) w_s[r] = row_w ? row_w[r0 + r] : 1u;
  if (tid == 0) nf_s = 0;
  // the live prefixes of this channel's three fields: uniform addresses, so they sit in scalar registers
  unsigned pref[3][NS];
#pragma unroll
  for (int f = 0; f < 3; ++f)
#pragma unroll
    for (int j = 0; j < NS; ++j) pref[f][j] = FIRST ? 0u : live[((size_t)c * 3 + f) * kMaxQ + j];
  __syncthreads();

  int cur[3] = {-1, -1, -1};   // the run: bin (slot * 256 + digit, or -1 = no live prefix) and its summed weight
  u64 sum[3] = {0, 0, 0};
  unsigned nf = 0;
  auto add = [&](float h, float t, unsigned w) {
    if (!(finite_bits(h) && finite_bits(t))) {   // (bit tests, as the metric: such a pair is counted, never binned)
      ++nf;
      return;
    }
    const unsigned k[3] = {key_of(t), key_of(h), key_of(fabsf(h - t))};
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      int idx = (int)((k[f] >> shift) & 255u);
      if (!FIRST) {
        const unsigned p = k[f] >> (shift + 8);
        int s = -1;
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (j < 4 || (j & ~3) < nl[f]) s = p == pref[f][j] ? j : s;   // (groups of four behind a uniform branch)
        idx = s < 0 ? -1 : s * 256 + idx;
      }
      if (idx != cur[f]) {
        if (cur[f] >= 0) atomicAdd(&hist[f * NS * 256 + cur[f]], sum[f]);
        cur[f] = idx;
        sum[f] = 0;
      }
      sum[f] += w;
    }
  };

  const size_t cbase = (size_t)c * H * W;
  const size_t g0 = cbase + (size_t)r0 * W, g1 = cbase + (size_t)r1 * W;
  // [g0, a0) and [a1, g1) element by element, [a0, a1) as float4 (empty without vec)
  size_t a0 = g1, a1 = g1;
  if (vec) {
    a0 = min((g0 + 3) & ~(size_t)3, g1);
    a1 = max(g1 & ~(size_t)3, a0);
  }
  for (size_t e = g0 + tid; e < a0; e += kThreads) add(xh[e], x[e], w_s[(unsigned)(e - cbase) / (unsigned)W - r0]);
  for (size_t e = a1 + tid; e < g1; e += kThreads) add(xh[e], x[e], w_s[(unsigned)(e - cbase) / (unsigned)W - r0]);

  const float4 *__restrict__ xh4 = reinterpret_cast<const float4 *>(xh);
  const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
  const size_t q1 = a1 / 4;
  size_t q = a0 / 4 + tid;
  auto body = [&](const float4 &h, const float4 &t, size_t qq) {
    const unsigned l = (unsigned)(4 * qq - cbase);   // element index inside the channel plane
    const unsigned row = l / (unsigned)W;
    const unsigned rem = l - row * (unsigned)W;
    const unsigned w0 = w_s[row - r0];
    // a float4 crosses into the next row only when W % 4 != 0; that row is then inside the band (the float4 is)
    const unsigned w1 = rem + 3 >= (unsigned)W ? w_s[row + 1 - r0] : w0;
    add(h.x, t.x, w0);
    add(h.y, t.y, rem + 1 >= (unsigned)W ? w1 : w0);
    add(h.z, t.z, rem + 2 >= (unsigned)W ? w1 : w0);
    add(h.w, t.w, w1);
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

#pragma unroll
  for (int f = 0; f < 3; ++f)
    if (cur[f] >= 0) atomicAdd(&hist[f * NS * 256 + cur[f]], sum[f]);
  if (FIRST && nf) atomicAdd(&nf_s, nf);
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 3; ++f)
    for (int i = tid; i < nlmax * 256; i += kThreads) {
      const u64 v = hist[f * NS * 256 + i];
      if (v) atomicAdd(&hist_g[((size_t)c * 3 + f) * gs * 256 + i], v);
    }
  if (FIRST && tid == 0 && nf_s) atomicAdd(&nonfinite_g[c], nf_s);
}

// One wave per (channel, field): lane l owns bins 4 l .. 4 l + 3 of a slot.  For every quantile: the digit whose
// cumulative weight first reaches the remaining target; then the distinct new prefixes become the next pass's slots.
// last: the prefixes are the keys of the answers - out [3][C][Q] and, behind it, the [C] non-finite counts.
__global__ __launch_bounds__(64) void quantile_select_kernel(Ws ws, int gs, int C, int Q, int last,
                                                             double *__restrict__ out) {
  __shared__ unsigned newp[kMaxQ], lv[kMaxQ];
  const int cf = blockIdx.x, lane = threadIdx.x;
  const int c = cf / 3, f = cf - c * 3;
  const size_t sb = (size_t)cf * kMaxQ;
  const int n = (int)ws.nlive[cf];
  for (int q = 0; q < Q; ++q) {
    const u64 T = ws.rem[sb + q];
    const unsigned old = ws.prefix[sb + q];
    const u64 *hb = ws.hist + ((size_t)cf * gs + ws.slot[sb + q]) * 256 + lane * 4;
    const u64 bin[4] = {hb[0], hb[1], hb[2], hb[3]};
    const u64 tot = bin[0] + bin[1] + bin[2] + bin[3];
    u64 inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 v = __shfl_up(inc, off, 64);
      inc += lane >= off ? v : 0;
    }
    u64 below = inc - tot;
    const bool hit = below < T && T <= inc;
    if (hit) {
      int d = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const bool more = d == i && below + bin[i] < T;
        below += more ? bin[i] : 0;
        d += more ? 1 : 0;
      }
      newp[q] = (old << 8) | (unsigned)(lane * 4 + d);
      ws.rem[sb + q] = T - below;
    }
    // no bin reaches the target only where non-finite pairs were left out: that channel reports NaN
    if (!__ballot(hit) && lane == 0) newp[q] = old << 8;
  }
  __syncthreads();
  if (last) {
    if (lane < Q) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      out[((size_t)f * C + c) * Q + lane] = ws.nonfinite[c] ? nan : (double)value_of(newp[lane]);
    }
    if (f == 0 && lane == 0) out[(size_t)3 * C * Q + c] = (double)ws.nonfinite[c];
    return;
  }
  for (int s = 0; s < n; ++s) {
    u64 *hb = ws.hist + ((size_t)cf * gs + s) * 256 + lane * 4;
    hb[0] = hb[1] = hb[2] = hb[3] = 0;
  }
  if (lane < Q) ws.prefix[sb + lane] = newp[lane];
  if (lane == 0) {
    int m = 0;
    for (int q = 0; q < Q; ++q) {
      int s = 0;
      while (s < m && lv[s] != newp[q]) ++s;
      if (s == m) lv[m++] = newp[q];
      ws.slot[sb + q] = (unsigned)s;
    }
    for (int s = 0; s < kMaxQ; ++s) ws.live[sb + s] = s < m ? lv[s] : kNoPrefix;
    ws.nlive[cf] = (unsigned)m;
  }
}

bool dims_ok(int C, int H, int W) {
  if (!(C > 0 && H > 0 && W > 0 && (size_t)H * W <= 0x7fffffffu)) return false;
  const int rows = band_rows(W);
  return (size_t)C * ((H + rows - 1) / rows) <= 0x7fffffffu && (size_t)C * 3 <= 0x7fffffffu;
}

template <int NS>
void launch_count(bool first, dim3 grid, hipStream_t st, const float *xh, const float *x, int H, int W, int rows, int bands,
                  const unsigned *row_w, int vec, int shift, const Ws &ws, int gs) {
  if (first)
    hipLaunchKernelGGL((quantile_count_kernel<1, true>), grid, dim3(threads_for(1)), 0, st, xh, x, H, W, rows, bands, row_w,
                       vec, shift, ws.live, ws.nlive, gs, ws.hist, ws.nonfinite);
  else
    hipLaunchKernelGGL((quantile_count_kernel<NS, false>), grid, dim3(threads_for(NS)), 0, st, xh, x, H, W, rows, bands,
                       row_w, vec, shift, ws.live, ws.nlive, gs, ws.hist, ws.nonfinite);
}

}  // namespace

extern "C" {

size_t cra5_frame_quantiles_ws_bytes(int C, int H, int W, int Q) {
  if (!dims_ok(C, H, W) || Q < 1 || Q > kMaxQ) return 0;
  return ws_layout(C, slots_for(Q), nullptr, nullptr);
}

int cra5_frame_quantiles_f32(const float *x_hat, const float *x, int C, int H, int W, const uint32_t *row_w,
                             const uint64_t *targets, int Q, void *ws, size_t ws_bytes, double *out, void *stream) {
  if (!x_hat || !x || !targets || !ws || !out || !dims_ok(C, H, W) || Q < 1 || Q > kMaxQ) return CRA5_ERR_ARG;
  if (ws_bytes < cra5_frame_quantiles_ws_bytes(C, H, W, Q) || ((uintptr_t)ws % 8) != 0) return CRA5_ERR_ARG;
  const int NS = slots_for(Q);
  Ws w;
  ws_layout(C, NS, ws, &w);
  const int rows = band_rows(W);
  const int bands = (H + rows - 1) / rows;
  const int vec = W >= 4 && ((uintptr_t)x_hat % 16) == 0 && ((uintptr_t)x % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t hist_n = (size_t)C * 3 * NS * 256;
  const size_t init_blocks = (hist_n + 255) / 256;
  hipLaunchKernelGGL(quantile_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(256), 0, st, w,
                     hist_n, C, Q, (const u64 *)targets);
  const dim3 grid(C * bands);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const bool first = pass == 0;
    switch (NS) {
      case 1: launch_count<1>(first, grid, st, x_hat, x, H, W, rows, bands, row_w, vec, shift, w, NS); break;
      case 2: launch_count<2>(first, grid, st, x_hat, x, H, W, rows, bands, row_w, vec, shift, w, NS); break;
      case 4: launch_count<4>(first, grid, st, x_hat, x, H, W, rows, bands, row_w, vec, shift, w, NS); break;
      case 8: launch_count<8>(first, grid, st, x_hat, x, H, W, rows, bands, row_w, vec, shift, w, NS); break;
      default: launch_count<16>(first, grid, st, x_hat, x, H, W, rows, bands, row_w, vec, shift, w, NS); break;
    }
    hipLaunchKernelGGL(quantile_select_kernel, dim3(C * 3), dim3(64), 0, st, w, NS, C, Q, pass == 3 ? 1 : 0, out);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
