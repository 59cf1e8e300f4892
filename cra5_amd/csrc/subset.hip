// Subset decode (VAEformer._decode_frame with `channels` / `box`): the two layout kernels around the unchanged fused
// un-embed.  The decoder's transformer runs on the whole token grid; the un-embed then runs on a patch-aligned superset
// of the requested lat/lon box only ("Subset decode"):
//   * cra5_gather_token_rows copies the superset's token rows of the final LayerNorm's output, verbatim (split-f16,
//     plain f16 or fp32 rows: bytes), wrapping the token columns at the grid's east edge;
//   * cra5_crop_f32 cuts the exact box out of the superset image, wrapping its columns when the superset is the full
//     circle.
// Both are pure copies: the values that reach the box are the full decode's, bit for bit.
// Thinned decode (`step`: every s_lat-th row / s_lon-th column of the global grid; subset.stride_plan): the tokens fall
// into classes that share one set of kept taps, and each class pair is one small GEMM:
//   * cra5_gather_token_lattice copies a class's token rows - a strided lattice of the token grid - verbatim;
//   * cra5_strided_scatter_f32 assembles the thinned image from the class matrices, one thread per output point: a seam
//     row's point is upper + lower partner in that order, then every point is de-normalised - the arithmetic of the full
//     decode's stores (gemm_split_epilogue_unembed.inc, unembed_fixup_kernel, col2im).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

// dst row r = superset token (i, j) = (r / n_tj, r % n_tj) <- src row (ti0 + i) * Wp + (tj0 + j) mod Wp; 16-byte units
__global__ __launch_bounds__(256) void gather_token_rows_kernel(const uint4 *__restrict__ src, size_t src_pitch16,
                                                                uint4 *__restrict__ dst, size_t dst_pitch16,
                                                                size_t row16, int Wp, int ti0, int tj0, int n_tj,
                                                                size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / row16, q = e - r * row16;
    const int i = (int)(r / n_tj), j = (int)(r - (size_t)i * n_tj);
    int tj = tj0 + j;
    if (tj >= Wp) tj -= Wp;   // (tj0 < Wp, j < n_tj <= Wp)
    dst[r * dst_pitch16 + q] = src[((size_t)(ti0 + i) * Wp + tj) * src_pitch16 + q];
  }
}

// dst[c][i][j] = src[c][r0 + i][(c0 + j) mod Ws]: one thread per output element, scalar accesses (any offset, any width)
__global__ __launch_bounds__(256) void crop_kernel(const float *__restrict__ src, int Hs, int Ws, float *__restrict__ dst,
                                                   int r0, int Hb, int c0, int Wb, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(e % Wb);
    const size_t t = e / Wb;
    const int i = (int)(t % Hb);
    const size_t c = t / Hb;
    int w = c0 + j;
    if (w >= Ws) w -= Ws;     // (c0 < Ws, j < Wb <= Ws)
    dst[e] = src[(c * Hs + (size_t)(r0 + i)) * Ws + w];
  }
}

// dst row r = class token (i, j) = (r / n_tj, r % n_tj) <- src row (ti0 + i * ti_step) * Wp + (tj0 + j * tj_step) mod Wp
__global__ __launch_bounds__(256) void gather_token_lattice_kernel(const uint4 *__restrict__ src, size_t src_pitch16,
                                                                   uint4 *__restrict__ dst, size_t dst_pitch16,
                                                                   size_t row16, int Wp, int ti0, int ti_step, int tj0,
                                                                   int tj_step, int n_tj, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / row16, q = e - r * row16;
    const int i = (int)(r / n_tj), j = (int)(r - (size_t)i * n_tj);
    int tj = tj0 + j * tj_step;
    if (tj >= Wp) tj -= Wp;   // (tj0 < Wp, j * tj_step < Wp: the launcher checks both)
    dst[r * dst_pitch16 + q] = src[((size_t)(ti0 + i * ti_step) * Wp + tj) * src_pitch16 + q];
  }
}

// Thinned image x[c][i][j] from the class matrices in the workspace g (subset.scatter_tables).  rows[i] = (rc, ti, ky)
// of the point's contribution(s) - two for a seam row, the upper partner first -, cols[j] = (cc, tj, kx), cls[rc * n_cc
// + cc] = (offset, pitch, n_tj, n_kx, n_ky * n_kx) of class matrix G: its element [ti * n_tj + tj][(c * n_ky + ky) * n_kx
// + kx].  One block per (channel, output row) - the row's table entries are block-uniform -, threads along the output
// row: coalesced stores; the scattered 4-byte reads hit matrices 1 / (s_lat * s_lon) of the frame's size.  An offset
// or a class
// index outside the workspace / the tables (tables that do not belong to it) reads nothing and stores a NaN.
__global__ __launch_bounds__(256) void strided_scatter_kernel(const float *__restrict__ g, size_t g_elems,
                                                              const int *__restrict__ rows, const int *__restrict__ cols,
                                                              const long long *__restrict__ cls, int n_rc, int n_cc,
                                                              const float *__restrict__ mean,
                                                              const float *__restrict__ stdv, float *__restrict__ x,
                                                              int C, int Ho, int Wo) {
  const size_t n_rows = (size_t)C * Ho;
  for (size_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int c = (int)(row / Ho), i = (int)(row - (size_t)c * Ho);
    const int *rt = rows + 6 * i;
    const int rc0 = rt[0], ti0 = rt[1], ky0 = rt[2], rc1 = rt[3], ti1 = rt[4], ky1 = rt[5];
    const float m = mean ? mean[c] : 0.f, sd = mean ? stdv[c] : 1.f;
    for (int j = threadIdx.x; j < Wo; j += blockDim.x) {
      const int cc = cols[3 * j], tj = cols[3 * j + 1], kx = cols[3 * j + 2];
      if (rc0 < 0 || rc0 >= n_rc || rc1 >= n_rc || cc < 0 || cc >= n_cc) {
        x[row * Wo + j] = __builtin_nanf("");
        continue;
      }
      const long long *k0 = cls + 5 * ((size_t)rc0 * n_cc + cc);
      const size_t o0 = (size_t)k0[0] + ((size_t)ti0 * k0[2] + tj) * k0[1] + (size_t)c * k0[4] + (size_t)ky0 * k0[3] + kx;
      float v = o0 < g_elems ? g[o0] : __builtin_nanf("");
      if (rc1 >= 0) {
        const long long *k1 = cls + 5 * ((size_t)rc1 * n_cc + cc);
        const size_t o1 = (size_t)k1[0] + ((size_t)ti1 * k1[2] + tj) * k1[1] + (size_t)c * k1[4] + (size_t)ky1 * k1[3] + kx;
        v = v + (o1 < g_elems ? g[o1] : __builtin_nanf(""));
      }
      if (mean) v = v * sd + m;
      x[row * Wo + j] = v;
    }
  }
}

unsigned blocks_for(size_t total) {
  const size_t g = (total + 255) / 256;
  return (unsigned)(g < 16384 ? (g ? g : 1) : 16384);
}

}  // namespace

extern "C" int cra5_gather_token_rows(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes,
                                      size_t row_bytes, int Hp, int Wp, int ti0, int n_ti, int tj0, int n_tj,
                                      void *stream) {
  if (!src || !dst || row_bytes == 0 || (row_bytes % 16) || (src_pitch_bytes % 16) || (dst_pitch_bytes % 16))
    return CRA5_ERR_ARG;
  if (src_pitch_bytes < row_bytes || dst_pitch_bytes < row_bytes) return CRA5_ERR_ARG;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return CRA5_ERR_ARG;
  if (Hp <= 0 || Wp <= 0 || ti0 < 0 || n_ti <= 0 || ti0 > Hp - n_ti || tj0 < 0 || tj0 >= Wp || n_tj <= 0 || n_tj > Wp)
    return CRA5_ERR_ARG;
  const size_t row16 = row_bytes / 16, total = (size_t)n_ti * n_tj * row16;
  hipLaunchKernelGGL(gather_token_rows_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4 *)src, src_pitch_bytes / 16, (uint4 *)dst, dst_pitch_bytes / 16, row16, Wp, ti0, tj0,
                     n_tj, total);
  return (int)hipGetLastError();
}

extern "C" int cra5_crop_f32(const float *src, int C, int Hs, int Ws, float *dst, int r0, int Hb, int c0, int Wb,
                             void *stream) {
  if (!src || !dst || C <= 0 || Hs <= 0 || Ws <= 0 || Hb <= 0 || Wb <= 0) return CRA5_ERR_ARG;
  if (r0 < 0 || r0 > Hs - Hb || c0 < 0 || c0 >= Ws || Wb > Ws) return CRA5_ERR_ARG;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3)) return CRA5_ERR_ARG;
  const size_t total = (size_t)C * Hb * Wb;
  hipLaunchKernelGGL(crop_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, dst, r0, Hb,
                     c0, Wb, total);
  return (int)hipGetLastError();
}

extern "C" int cra5_gather_token_lattice(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes,
                                         size_t row_bytes, int Hp, int Wp, int ti0, int ti_step, int n_ti, int tj0,
                                         int tj_step, int n_tj, void *stream) {
  if (!src || !dst || row_bytes == 0 || (row_bytes % 16) || (src_pitch_bytes % 16) || (dst_pitch_bytes % 16))
    return CRA5_ERR_ARG;
  if (src_pitch_bytes < row_bytes || dst_pitch_bytes < row_bytes) return CRA5_ERR_ARG;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return CRA5_ERR_ARG;
  if (Hp <= 0 || Wp <= 0 || ti0 < 0 || ti0 >= Hp || ti_step <= 0 || n_ti <= 0 || tj0 < 0 || tj0 >= Wp || tj_step <= 0 ||
      n_tj <= 0)
    return CRA5_ERR_ARG;
  // the last token row lies inside the grid; the token columns wrap at most once and name no token twice
  if ((long long)ti0 + (long long)(n_ti - 1) * ti_step >= Hp || (long long)(n_tj - 1) * tj_step >= Wp) return CRA5_ERR_ARG;
  const size_t row16 = row_bytes / 16, total = (size_t)n_ti * n_tj * row16;
  hipLaunchKernelGGL(gather_token_lattice_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4 *)src, src_pitch_bytes / 16, (uint4 *)dst, dst_pitch_bytes / 16, row16, Wp, ti0,
                     ti_step, tj0, tj_step, n_tj, total);
  return (int)hipGetLastError();
}

extern "C" int cra5_strided_scatter_f32(const float *g, size_t g_elems, const int *rows, const int *cols,
                                        const long long *cls, int n_rc, int n_cc, const float *mean, const float *stdv,
                                        float *x, int C, int Ho, int Wo, void *stream) {
  if (!g || !g_elems || !rows || !cols || !cls || !x || n_rc <= 0 || n_cc <= 0 || C <= 0 || Ho <= 0 || Wo <= 0)
    return CRA5_ERR_ARG;
  if ((mean == nullptr) != (stdv == nullptr)) return CRA5_ERR_ARG;
  if (((uintptr_t)g & 3) || ((uintptr_t)x & 3) || ((uintptr_t)rows & 3) || ((uintptr_t)cols & 3) || ((uintptr_t)cls & 7))
    return CRA5_ERR_ARG;
  const size_t n_rows = (size_t)C * Ho;
  hipLaunchKernelGGL(strided_scatter_kernel, dim3((unsigned)(n_rows < 65535 ? n_rows : 65535)), dim3(Wo > 128 ? 256 : 128),
                     0, (hipStream_t)stream, g, g_elems, rows, cols, cls, n_rc, n_cc, mean, stdv, x, C, Ho, Wo);
  return (int)hipGetLastError();
}
