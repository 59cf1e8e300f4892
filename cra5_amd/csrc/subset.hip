// Subset decode (VAEformer._decode_frame with `channels` / `box`): the two layout kernels around the unchanged fused
// un-embed.  The decoder's transformer runs on the whole token grid; the un-embed then runs on a patch-aligned superset
// of the requested lat/lon box only ("Subset decode"):
//   * cra5_gather_token_rows copies the superset's token rows of the final LayerNorm's output, verbatim (split-f16,
//     plain f16 or fp32 rows: bytes), wrapping the token columns at the grid's east edge;
//   * cra5_crop_f32 cuts the exact box out of the superset image, wrapping its columns when the superset is the full
//     circle.
// Both are pure copies: the values that reach the box are the full decode's, bit for bit.
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
