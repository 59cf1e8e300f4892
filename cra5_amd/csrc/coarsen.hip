// Area-weighted coarsening (cra5_amd/subset.py coarsen_plan; DESIGN.md section 4, "Coarsening"): the first-order
// conservative regrid of a decoded frame onto every k_lat-th row / k_lon-th column of the global grid, one streaming pass.
//
//   out[c][i][j] = (float) sum over the window's rows h = row0[i] + t, north to south, of rw[i][t] * inner(h, col_j)
//   inner(h, col) = sum over the window's columns w = col - k_lon / 2 .. col + k_lon / 2 (mod W), west to east, of
//                   ov * (double)x[h][w],   ov = 1/2 on the two edge columns of an even k_lon, 1 elsewhere
//
// in float64, every sum starting from 0, every add and the one product per row rounded on its own (contraction off; ov *
// x is exact).  inner depends on the GLOBAL (h, col) only and the row sum on the global output row only: a region's
// result is the sub-block of the globe's, bit for bit.
//
// One block = one channel x a tile of <= 256 output columns x a run of output rows, walked north to south.  Per source
// row the block stages the tile's span - (tile columns - 1) * k_lon + 2 * (k_lon / 2) + 1 floats, at most two contiguous
// pieces when it crosses the source's east edge - in LDS with 16-byte loads (the pieces' first / last partial quads go
// element by element: any 4-byte aligned base works), and the loads of the NEXT row are issued before the current row is
// reduced, so they fly under the LDS reads and the fp64 adds.  Each thread owns one output column: it reads its k_lon (+
// 1) floats from LDS and keeps the row sum in a register.  Index i lives at dword i + i / 32.  By the bank rule of a
// 4-byte LDS read (bank = dword mod 32, conflicts counted inside each 32-lane half) a lane stride of k_lon dwords is
// gcd(k_lon, 32)-way conflicted unpadded: 2-way at k_lon = 2, 6, 10, 4-way at 4 and 12, 8-way at 8 and 24, 32-way at 32,
// none at an odd k_lon.  With the padding every k_lon from 2 to 32 is at most 2-way, on some of the k_lon + 1 reads (an odd
// k_lon pays for it: none -> 2-way).  The degree is computed from the rule, not measured with a counter.  The edge row two output rows share (even k_lat) is staged and reduced ONCE - its
// inner is kept for the next output row - and the edge column two outputs share is read from LDS twice, from HBM once.
// Rows come from device tables: a row outside the source is not read, its output becomes NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAXQ = 8;                          // 16-byte loads in flight per thread and row
constexpr int SPAN_MAX = THREADS * MAXQ * 4 - 16; // floats of one staged row: each of two pieces may open and close a partial quad

struct Geo {
  int Hs, Ws, src_r0, src_c0, W;          // source [.][Hs][Ws], its first global row / column
  int k_lat, Ho, k_lon, Wo, col0;         // output progression: column j = (col0 + j * k_lon) mod W
  int rw_pitch, tile_cols, n_tiles, rows_per_block, n_chunks;
};

__device__ __forceinline__ int lds_at(int i) { return i + (i >> 5); }

// The staged span of one source row: piece 0 = n0 floats from local column l0, piece 1 = n1 floats from local column 0
// (the part past the east edge of a whole-circle source).  Quad q of a piece covers elements 4 q - mis .. + 3 of it,
// mis = the piece's first element's offset inside its 16-byte line.
struct Span {
  int l0, n0, n1, mis0, nq0, mis1, nq1;
};

__device__ __forceinline__ void issue_row(const float *__restrict__ row, const Span &s, float4 (&r)[MAXQ]) {
#pragma unroll
  for (int v = 0; v < MAXQ; ++v) {
    int q = (int)threadIdx.x + v * THREADS;
    const float *p;
    int n, mis;
    if (q < s.nq0) {
      p = row + s.l0, n = s.n0, mis = s.mis0;
    } else if (q < s.nq0 + s.nq1) {
      q -= s.nq0, p = row, n = s.n1, mis = s.mis1;
    } else {
      continue;
    }
    const int e = 4 * q - mis;
    if (e >= 0 && e + 4 <= n) {
      r[v] = *reinterpret_cast<const float4 *>(p + e);
    } else {
      r[v].x = (e >= 0 && e < n) ? p[e] : 0.f;
      r[v].y = (e + 1 >= 0 && e + 1 < n) ? p[e + 1] : 0.f;
      r[v].z = (e + 2 >= 0 && e + 2 < n) ? p[e + 2] : 0.f;
      r[v].w = (e + 3 >= 0 && e + 3 < n) ? p[e + 3] : 0.f;
    }
  }
}

__device__ __forceinline__ void commit_row(float *__restrict__ lds, const Span &s, const float4 (&r)[MAXQ]) {
#pragma unroll
  for (int v = 0; v < MAXQ; ++v) {
    int q = (int)threadIdx.x + v * THREADS;
    int n, base, mis;
    if (q < s.nq0) {
      n = s.n0, base = 0, mis = s.mis0;
    } else if (q < s.nq0 + s.nq1) {
      q -= s.nq0, n = s.n1, base = s.n0, mis = s.mis1;
    } else {
      continue;
    }
    const int e = 4 * q - mis;
    if (e >= 0 && e < n) lds[lds_at(base + e)] = r[v].x;
    if (e + 1 >= 0 && e + 1 < n) lds[lds_at(base + e + 1)] = r[v].y;
    if (e + 2 >= 0 && e + 2 < n) lds[lds_at(base + e + 2)] = r[v].z;
    if (e + 3 >= 0 && e + 3 < n) lds[lds_at(base + e + 3)] = r[v].w;
  }
}

__global__ __launch_bounds__(THREADS) void coarsen_kernel(const float *__restrict__ src, const int *__restrict__ row0,
                                                          const int *__restrict__ ntap, const double *__restrict__ rw,
                                                          const int *__restrict__ chan_map, int C_src,
                                                          float *__restrict__ dst, Geo g) {
  extern __shared__ float lds[];
  const int tile = (int)(blockIdx.x % (unsigned)g.n_tiles);
  const unsigned rest = blockIdx.x / (unsigned)g.n_tiles;
  const int chunk = (int)(rest % (unsigned)g.n_chunks);
  const int c_out = (int)(rest / (unsigned)g.n_chunks);
  const int c_src = chan_map ? chan_map[c_out] : c_out;
  const bool chan_ok = c_src >= 0 && c_src < C_src;

  const int j0 = tile * g.tile_cols;
  const int ncol = min(g.tile_cols, g.Wo - j0);
  const int half = g.k_lon / 2, nwin = 2 * half + 1;
  const bool halves = half > 0 && (g.k_lon & 1) == 0;
  const int n_span = (ncol - 1) * g.k_lon + nwin;

  // the span's first global column -> local column of the source (the launcher checked that the span stays inside it)
  long long first = ((long long)g.col0 + (long long)j0 * g.k_lon - half - g.src_c0) % g.W;
  if (first < 0) first += g.W;
  Span s;
  s.l0 = (int)first;
  s.n0 = min(n_span, g.Ws - s.l0);
  s.n1 = n_span - s.n0;                 // > 0 only on a whole-circle source
  const float *chan = src + (size_t)(chan_ok ? c_src : 0) * g.Hs * g.Ws;

  const int i0 = chunk * g.rows_per_block, i1 = min(g.Ho, i0 + g.rows_per_block);
  const int j = (int)threadIdx.x;
  const bool owner = j < ncol;
  float *out = dst + ((size_t)c_out * g.Ho) * g.Wo + j0 + j;

  float4 r[MAXQ];
  int i = i0, t = 0;
  int nt_i = min(max(ntap[i], 0), g.rw_pitch);
  int h = row0[i];                       // the row in LDS (or about to be)
  bool h_ok = chan_ok && nt_i > 0 && h >= g.src_r0 && h < g.src_r0 + g.Hs;
  bool bad = !h_ok;                      // the output row under way touched a row outside the source
  auto spans_of = [&](int hh) {
    const float *row = chan + (size_t)(hh - g.src_r0) * g.Ws;
    s.mis0 = (int)(((uintptr_t)(row + s.l0) >> 2) & 3);
    s.nq0 = (s.mis0 + s.n0 + 3) >> 2;
    s.mis1 = (int)(((uintptr_t)row >> 2) & 3);
    s.nq1 = s.n1 > 0 ? (s.mis1 + s.n1 + 3) >> 2 : 0;
    return row;
  };
  if (h_ok) {
    const float *row = spans_of(h);
    issue_row(row, s, r);
    commit_row(lds, s, r);
  }
  __syncthreads();
  double acc = 0.0, inner = 0.0;
  bool fresh = true;                     // LDS holds a row whose inner is not computed yet
  while (i < i1) {
    // the next (output row, tap) and its source row
    int ni = i, nt = t + 1;
    if (nt >= nt_i) ni = i + 1, nt = 0;
    int nnt_i = nt_i, nh = -1;
    if (ni < i1) {
      if (ni != i) nnt_i = min(max(ntap[ni], 0), g.rw_pitch);
      nh = row0[ni] + nt;
    }
    const bool load = ni < i1 && nnt_i > 0 && nh != h;
    const bool nh_ok = chan_ok && nh >= g.src_r0 && nh < g.src_r0 + g.Hs;
    Span sn = s;
    if (load && nh_ok) {
      const float *row = spans_of(nh);
      sn = s;
      issue_row(row, sn, r);             // in flight while this row is reduced
    }
    if (fresh && owner && h_ok) {
      const int b = j * g.k_lon;
      double in = 0.0;
      if (halves) {
        in = in + 0.5 * (double)lds[lds_at(b)];
        for (int w = 1; w < nwin - 1; ++w) in = in + (double)lds[lds_at(b + w)];
        in = in + 0.5 * (double)lds[lds_at(b + nwin - 1)];
      } else {
        for (int w = 0; w < nwin; ++w) in = in + (double)lds[lds_at(b + w)];
      }
      inner = in;
    }
    fresh = false;
    if (nt_i > 0) {
      if (!h_ok) bad = true;
      acc = acc + rw[(size_t)i * g.rw_pitch + t] * inner;
    }
    if (ni != i) {                       // the output row is complete
      if (owner) out[(size_t)i * g.Wo] = (bad || nt_i <= 0) ? __builtin_nanf("") : (float)acc;
      acc = 0.0;
      bad = false;
    }
    if (load) {
      __syncthreads();                   // every thread has read the row in LDS
      if (nh_ok) commit_row(lds, sn, r);
      __syncthreads();
      h = nh, h_ok = nh_ok, fresh = true;
    }
    i = ni, t = nt, nt_i = nnt_i;
  }
}

}  // namespace

extern "C" int cra5_coarsen_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W,
                                int whole_circle, int out_r0, int k_lat, int Ho, int out_c0, int k_lon, int Wo,
                                const int *row0, const int *ntap, const double *rw, int rw_pitch, const int *chan_map,
                                int C_out, float *dst, void *stream) {
  if (!src || !dst || !row0 || !ntap || !rw) return CRA5_ERR_ARG;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row0 & 3) || ((uintptr_t)ntap & 3) ||
      ((uintptr_t)rw & 7) || ((uintptr_t)chan_map & 3))
    return CRA5_ERR_ARG;
  if (C_src <= 0 || C_out <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || k_lat <= 0 ||
      k_lon <= 0 || rw_pitch <= 0)
    return CRA5_ERR_ARG;
  if (!chan_map && C_out > C_src) return CRA5_ERR_ARG;
  if (src_r0 < 0 || Hs > H - src_r0 || src_c0 < 0 || src_c0 >= W || Ws > W) return CRA5_ERR_ARG;
  if (whole_circle ? (Ws != W || src_c0 != 0) : false) return CRA5_ERR_ARG;
  if (out_c0 < 0 || out_c0 >= W || (long long)Wo * k_lon > W) return CRA5_ERR_ARG;
  // rows: the windows out_r0 + i * k_lat -+ k_lat / 2, clipped at the poles, lie inside the source
  const long long r_last = (long long)out_r0 + (long long)(Ho - 1) * k_lat;
  if (out_r0 < 0 || r_last > H - 1) return CRA5_ERR_ARG;
  const long long top = out_r0 - k_lat / 2 > 0 ? out_r0 - k_lat / 2 : 0;
  const long long bot = r_last + k_lat / 2 < H - 1 ? r_last + k_lat / 2 : H - 1;
  if (top < src_r0 || bot > (long long)src_r0 + Hs - 1) return CRA5_ERR_ARG;
  // columns: the span of all windows, eastward from out_c0 - k_lon / 2
  const int half = k_lon / 2;
  const long long span = (long long)(Wo - 1) * k_lon + 2 * half + 1;
  if (!whole_circle) {
    long long off = ((long long)out_c0 - half - src_c0) % W;
    if (off < 0) off += W;
    if (off + span > Ws) return CRA5_ERR_ARG;
  }
  if ((long long)k_lon + 1 > SPAN_MAX) return CRA5_ERR_ARG;

  Geo g;
  g.Hs = Hs, g.Ws = Ws, g.src_r0 = src_r0, g.src_c0 = src_c0, g.W = W;
  g.k_lat = k_lat, g.Ho = Ho, g.k_lon = k_lon, g.Wo = Wo, g.col0 = out_c0, g.rw_pitch = rw_pitch;
  int tc = (SPAN_MAX - 2 * half - 1) / k_lon + 1;       // (tc - 1) * k_lon + 2 * half + 1 <= SPAN_MAX
  if (tc > THREADS) tc = THREADS;
  if (tc > Wo) tc = Wo;
  g.tile_cols = tc;
  g.n_tiles = (Wo + tc - 1) / tc;
  // enough blocks to fill the chip several times over; a longer run of rows re-reads fewer shared edge rows
  const long long per_row = (long long)C_out * g.n_tiles;
  long long chunks = (4096 + per_row - 1) / per_row;
  if (chunks > Ho) chunks = Ho;
  if (chunks < 1) chunks = 1;
  g.rows_per_block = (int)((Ho + chunks - 1) / chunks);
  g.n_chunks = (Ho + g.rows_per_block - 1) / g.rows_per_block;
  const long long blocks = per_row * g.n_chunks;
  if (blocks > 0x7fffffffLL) return CRA5_ERR_ARG;
  const int n_span = (tc - 1) * k_lon + 2 * half + 1;
  const size_t lds_bytes = (size_t)(n_span + (n_span >> 5) + 1) * sizeof(float);
  hipLaunchKernelGGL(coarsen_kernel, dim3((unsigned)blocks), dim3(THREADS), lds_bytes, (hipStream_t)stream, src, row0, ntap,
                     rw, chan_map, C_src, dst, g);
  return (int)hipGetLastError();
}
