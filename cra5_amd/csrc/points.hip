// Point decode (VAEformer._unembed_points; cra5_amd/points.py; DESIGN.md section 4 "Point sampling", section 10.7): the
// decoded frame at a list of (lat, lon) positions - stations, a track - without the frame.
//   * cra5_gather_token_list copies the token rows a point list needs out of the final LayerNorm's output, verbatim
//     (split-f16, plain f16 or fp32 rows: bytes), by a device list of token indexes;
//   * cra5_points_from_cols picks the points out of the two-call un-embed's column matrix of those tokens: a node is one
//     product, or upper + lower partner on a seam row, then de-normalised - the expression, order and contraction of
//     strided_scatter_kernel (csrc/subset.hip), whose bits are the full decode's;
//   * cra5_points_from_image picks them out of an image [C][H][W] that is already there.
// One kernel body, two node fetchers.  Nearest: the node's fp32 value, copied.  Bilinear: regridding's fixed arithmetic
// (csrc/window_reduce.hip) - float64, every sum from 0.0, every product and add rounded on its own, north to south over
// west to east:  out[c][p] = (float) sum_t rw[p][t] * (sum_u cw[p][u] * (double)v(node[p][t][u], c)).
// The tables live on the device: every index is checked before it is followed; an entry outside its source is never read
// and yields NaN.  Output [C][P], lanes along p: coalesced stores.  These kernels move kilobytes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

namespace {

// dst row r = src row tok[r], 16-byte units; an index outside [0, n_src_rows): nothing is read, the row is all 0xFF bytes
__global__ __launch_bounds__(256) void gather_token_list_kernel(const uint4 *__restrict__ src, size_t src_pitch16,
                                                                uint4 *__restrict__ dst, size_t dst_pitch16,
                                                                size_t row16, int n_src_rows,
                                                                const int *__restrict__ tok, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / row16, q = e - r * row16;
    const int t = tok[r];
    uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    if (t >= 0 && t < n_src_rows) v = src[(size_t)t * src_pitch16 + q];
    dst[r * dst_pitch16 + q] = v;
  }
}

// Node n of the column matrix cols [M][pitch]: channel c's products start at column c * tpc; nodes[n] = (m0, tap0, m1,
// tap1), m1 = -1: no second contribution.  The arithmetic is strided_scatter_kernel's, in its order, under this file's
// default contraction (the build's: the de-normalisation contracts as it does there).
struct ColsFetch {
  const float *cols;
  size_t pitch;
  int M, tpc;
  const int *nodes;
  int n_nodes;
  const float *mean, *stdv;

  __device__ __forceinline__ float operator()(int n, int, int c) const {
    if (n < 0 || n >= n_nodes) return __builtin_nanf("");
    const int m0 = nodes[4 * n], t0 = nodes[4 * n + 1], m1 = nodes[4 * n + 2], t1 = nodes[4 * n + 3];
    if (m0 < 0 || m0 >= M || t0 < 0 || t0 >= tpc || m1 >= M || (m1 >= 0 && (t1 < 0 || t1 >= tpc)))
      return __builtin_nanf("");
    float v = cols[(size_t)m0 * pitch + (size_t)c * tpc + t0];
    if (m1 >= 0) v = v + cols[(size_t)m1 * pitch + (size_t)c * tpc + t1];
    if (mean) v = v * stdv[c] + mean[c];
    return v;
  }
};

// Node (r, cc) of the image x [C][H][W]
struct ImageFetch {
  const float *x;
  int H, W;

  __device__ __forceinline__ float operator()(int r, int cc, int c) const {
    if (r < 0 || r >= H || cc < 0 || cc >= W) return __builtin_nanf("");
    return x[((size_t)c * H + r) * W + cc];
  }
};

// a[ts * p + 0..1], b[ts * p + 0..1]: the point's taps.  ColsFetch (ts = 4): a = the nodes of row tap 0, b = those of row
// tap 1 (entry u: column tap u; the fetcher's second argument is unused).  ImageFetch (ts = 2): a = the rows, b = the
// columns.  -1: no such tap.
template <class Fetch, bool kByNode>
__global__ __launch_bounds__(256) void points_kernel(Fetch f, const int *__restrict__ a, const int *__restrict__ b,
                                                     int ts, const double *__restrict__ rw,
                                                     const double *__restrict__ cw, int P, int nearest,
                                                     float *__restrict__ out) {
  const int c = (int)blockIdx.y;
  for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < P; p += (int)(gridDim.x * blockDim.x)) {
    const int a0 = a[ts * p], a1 = a[ts * p + 1], b0 = b[ts * p], b1 = b[ts * p + 1];
    float res;
    if (nearest) {
      res = kByNode ? f(a0, 0, c) : f(a0, b0, c);          // the node's bits, no arithmetic
    } else {
#pragma clang fp contract(off)
      // (row tap t, column tap u) -> the fetcher's arguments
      const int nt = kByNode ? 1 + (b0 != -1) : 1 + (a1 != -1);
      const int nu = kByNode ? 1 + (a1 != -1) : 1 + (b1 != -1);
      const double r0 = rw[2 * p], r1 = rw[2 * p + 1], c0 = cw[2 * p], c1 = cw[2 * p + 1];
      double acc = 0.0;
      for (int t = 0; t < nt; ++t) {
        double inner = 0.0;
        for (int u = 0; u < nu; ++u) {
          float v;
          if (kByNode)
            v = f(t == 0 ? (u == 0 ? a0 : a1) : (u == 0 ? b0 : b1), 0, c);
          else
            v = f(t == 0 ? a0 : a1, u == 0 ? b0 : b1, c);
          inner = inner + (u == 0 ? c0 : c1) * (double)v;
        }
        acc = acc + (t == 0 ? r0 : r1) * inner;
      }
      res = (float)acc;
    }
    out[(size_t)c * P + p] = res;
  }
}

unsigned blocks_for(size_t total) {
  const size_t g = (total + 255) / 256;
  return (unsigned)(g < 16384 ? (g ? g : 1) : 16384);
}

bool misaligned(const void *p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// what both point launchers share: the output's size, the weights' presence
bool points_args_ok(int C, int P, int nearest, const double *rw, const double *cw, const float *out) {
  if (!out || C <= 0 || C > 65535 || P <= 0 || (long long)C * P > INT_MAX) return false;
  if (!nearest && (!rw || !cw)) return false;
  return !(misaligned(out, 3) || misaligned(rw, 7) || misaligned(cw, 7));
}

}  // namespace

extern "C" int cra5_gather_token_list(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes,
                                      size_t row_bytes, int n_src_rows, const int *tok, int n_tok, void *stream) {
  if (!src || !dst || !tok || row_bytes == 0 || (row_bytes % 16) || (src_pitch_bytes % 16) || (dst_pitch_bytes % 16))
    return CRA5_ERR_ARG;
  if (src_pitch_bytes < row_bytes || dst_pitch_bytes < row_bytes) return CRA5_ERR_ARG;
  if (misaligned(src, 15) || misaligned(dst, 15) || misaligned(tok, 3)) return CRA5_ERR_ARG;
  if (n_src_rows <= 0 || n_tok <= 0) return CRA5_ERR_ARG;
  const size_t row16 = row_bytes / 16, total = (size_t)n_tok * row16;
  hipLaunchKernelGGL(gather_token_list_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4 *)src, src_pitch_bytes / 16, (uint4 *)dst, dst_pitch_bytes / 16, row16, n_src_rows, tok,
                     total);
  return (int)hipGetLastError();
}

extern "C" int cra5_points_from_cols(const float *cols, size_t pitch, int M, int C, int taps_per_channel, const int *nodes,
                                     int n_nodes, const int *pnode, const double *rw, const double *cw, int P, int nearest,
                                     const float *mean, const float *stdv, float *out, void *stream) {
  if (!cols || !nodes || !pnode || !points_args_ok(C, P, nearest, rw, cw, out)) return CRA5_ERR_ARG;
  if (M <= 0 || taps_per_channel <= 0 || n_nodes <= 0) return CRA5_ERR_ARG;
  if ((long long)C * taps_per_channel > INT_MAX || (size_t)C * taps_per_channel > pitch) return CRA5_ERR_ARG;
  if (pitch > (size_t)INT_MAX || (long long)n_nodes * 4 > INT_MAX || (long long)P * 4 > INT_MAX) return CRA5_ERR_ARG;
  if ((mean == nullptr) != (stdv == nullptr)) return CRA5_ERR_ARG;
  if (misaligned(cols, 3) || misaligned(nodes, 3) || misaligned(pnode, 3) || misaligned(mean, 3) || misaligned(stdv, 3))
    return CRA5_ERR_ARG;
  const ColsFetch f{cols, pitch, M, taps_per_channel, nodes, n_nodes, mean, stdv};
  const dim3 grid((unsigned)((P + 255) / 256 < 4096 ? (P + 255) / 256 : 4096), (unsigned)C);
  hipLaunchKernelGGL((points_kernel<ColsFetch, true>), grid, dim3(256), 0, (hipStream_t)stream, f, pnode, pnode + 2, 4,
                     rw, cw, P, nearest, out);
  return (int)hipGetLastError();
}

extern "C" int cra5_points_from_image(const float *x, int C, int H, int W, const int *rows, const int *cols,
                                      const double *rw, const double *cw, int P, int nearest, float *out, void *stream) {
  if (!x || !rows || !cols || !points_args_ok(C, P, nearest, rw, cw, out)) return CRA5_ERR_ARG;
  if (H <= 0 || W <= 0 || (long long)H * W > INT_MAX || (long long)P * 2 > INT_MAX) return CRA5_ERR_ARG;
  if (misaligned(x, 3) || misaligned(rows, 3) || misaligned(cols, 3)) return CRA5_ERR_ARG;
  const ImageFetch f{x, H, W};
  const dim3 grid((unsigned)((P + 255) / 256 < 4096 ? (P + 255) / 256 : 4096), (unsigned)C);
  hipLaunchKernelGGL((points_kernel<ImageFetch, false>), grid, dim3(256), 0, (hipStream_t)stream, f, rows, cols, 2, rw,
                     cw, P, nearest, out);
  return (int)hipGetLastError();
}
