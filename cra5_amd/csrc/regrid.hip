// Regridding onto any rectilinear lat/lon grid (cra5_amd/regrid.py Grid.plan; DESIGN.md section 4, "Regridding"): bilinear
// interpolation and first-order conservative remapping are ONE separable weighted reduction with per-row and per-column
// weight tables - coarsen.hip's reduction with its regular column windows replaced by a table.
//
//   inner(h, j)  = sum over u = 0 .. ctap[j] - 1, west to east,   of cw[j][u] * (double)x[h][(col0[j] + u) mod W]
//   out[c][i][j] = (float) sum over t = 0 .. ntap[i] - 1, north to south, of rw[i][t] * inner(row0[i] + t, j)
//
// in float64, every sum starting from 0, every product and every add rounded on its own (contraction off).  inner depends
// on the GLOBAL (h, j) only and a row sum on the target row only: results are bit-identical from run to run and a
// sub-grid's result is the sub-block of the whole target grid's.
//
// One block = one channel x one column tile x a run of target rows, walked north to south through `order` (the target
// rows sorted north to south; row order[k] is WRITTEN, so a south-to-north target comes back in the caller's order).  The
// tiles come from the host (regrid.tile_table): <= tile_cols consecutive target columns whose source span - the columns
// are monotone, so one eastward run, at most two pieces across the source's east edge - fits the staged-row budget.
// Per source row the block stages the span in LDS with 16-byte loads (partial first / last quads element by element: any
// 4-byte aligned base works; dword i lives at i + i / 32, coarsen.hip's padding), and the loads of the NEXT row to stage
// are issued before the current row is reduced.  Each thread owns one target column; its column weights sit in LDS
// ([tap][column]: conflict-free), loaded once per block - they never join the per-row HBM stream.  The inner of the two
// most recently staged source rows stay in registers, tagged by global row: bilinear at any ratio and conservative
// windows that share at most their edge row stage every source row once per block.
//
// Limits the launcher enforces.  ctap <= cw_pitch <= 64: a tile's column weights must fit 32 KB of LDS beside the 32 KB
// staged row (cw_pitch x tile columns x 8 bytes; 64 taps leave 64 columns per tile) - a 5.625 deg target on the 0.25 deg
// grid takes 23 or 24.  ntap <= rw_pitch <= H: rows are streamed, a window cannot hold more rows than the grid.  A
// staged span holds at most 7936 floats, and its piece past the source's east edge at most one row (W).
// The tables live on the device, so the kernel checks every entry before use: a row or a column window outside the
// source, a tile span outside the source or the budget, or a channel outside the source is never read - those outputs
// become NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAXQ = 8;                 // 16-byte loads in flight per thread and row
constexpr int SPAN_MAX = 7936;          // floats of one staged row: (n + n / 32 + 1) * 4 <= 32 KB, <= THREADS * MAXQ * 4 - 16
constexpr int CW_MAX_DOUBLES = 4096;    // cw_pitch * tile columns: 32 KB
constexpr int CTAP_MAX = 64;

struct Geo {
  int Hs, Ws, src_r0, src_c0, W, whole;   // source [.][Hs][Ws], its first global row / column; whole: Ws == W
  int Ho, Wo, rw_pitch, cw_pitch;
  int n_tiles, tile_cols, max_span, rows_per_block, n_chunks;
};

__device__ __forceinline__ int lds_at(int i) { return i + (i >> 5); }

// The staged span of one source row: piece 0 = n0 floats from local column l0, piece 1 = n1 floats from local column 0
// (the part past the east edge of a whole-circle source).  Quad q of a piece covers elements 4 q - mis .. + 3 of it.
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

// A position of the walk: tap t of the window of target row i = order[k].
struct Cur {
  int k, t, i, nt, r0;
};

__global__ __launch_bounds__(THREADS) void regrid_kernel(const float *__restrict__ src, const int *__restrict__ row0,
                                                         const int *__restrict__ ntap, const double *__restrict__ rw,
                                                         const int *__restrict__ order, const int *__restrict__ col0,
                                                         const int *__restrict__ ctap, const double *__restrict__ cw,
                                                         const int *__restrict__ tiles, const int *__restrict__ chan_map,
                                                         int C_src, float *__restrict__ dst, Geo g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *cwl = smem;                                                        // [cw_pitch][tile_cols]
  float *lds = reinterpret_cast<float *>(smem + (size_t)g.cw_pitch * g.tile_cols);
  const int tile = (int)(blockIdx.x % (unsigned)g.n_tiles);
  const unsigned rest = blockIdx.x / (unsigned)g.n_tiles;
  const int chunk = (int)(rest % (unsigned)g.n_chunks);
  const int c_out = (int)(rest / (unsigned)g.n_chunks);
  const int c_src = chan_map ? chan_map[c_out] : c_out;
  const bool chan_ok = c_src >= 0 && c_src < C_src;

  const int j0 = tiles[4 * tile], ncol = tiles[4 * tile + 1], first = tiles[4 * tile + 2], n_span = tiles[4 * tile + 3];
  if (j0 < 0 || ncol < 1 || ncol > g.tile_cols || ncol > g.Wo - j0) return;       // no column of dst is named
  // the span inside the source: local column l0, one piece or (whole circle) two
  Span s;
  bool span_ok = first >= 0 && first < g.W && n_span >= 1 && n_span <= g.max_span;
  int l0 = first - g.src_c0;
  if (l0 < 0) l0 += g.W;
  // the piece past the east edge starts again at column 0 and must end inside the row (it may pass l0: a span of a
  // whole circle plus a window stages a few columns twice)
  span_ok = span_ok && l0 >= 0 && l0 < g.Ws && (g.whole ? n_span - (g.Ws - l0) <= g.Ws : n_span <= g.Ws - l0);
  s.l0 = span_ok ? l0 : 0;
  s.n0 = span_ok ? min(n_span, g.Ws - s.l0) : 0;
  s.n1 = span_ok ? n_span - s.n0 : 0;                                        // > 0 only on a whole-circle source
  const float *chan = src + (size_t)(chan_ok ? c_src : 0) * g.Hs * g.Ws;

  // this thread's column: its window inside the staged span, its weights into LDS
  const int j = (int)threadIdx.x;
  const bool owner = j < ncol;
  int off = 0, ct = 0;
  bool col_ok = false;
  if (owner) {
    ct = ctap[j0 + j];
    off = col0[j0 + j] - first;
    if (off < 0) off += g.W;
    col_ok = span_ok && chan_ok && ct >= 1 && ct <= g.cw_pitch && off >= 0 && off <= n_span - ct;
    if (col_ok)
      for (int u = 0; u < ct; ++u) cwl[u * g.tile_cols + j] = cw[(size_t)(j0 + j) * g.cw_pitch + u];
  }
  float *out = dst + ((size_t)c_out * g.Ho) * g.Wo + j0 + j;
  const bool load_ok = span_ok && chan_ok;

  const int k0 = chunk * g.rows_per_block, k1 = min(g.Ho, k0 + g.rows_per_block);
  auto window = [&](Cur &c) {               // the window of walk position c.k
    c.i = -1, c.nt = 0, c.r0 = 0;
    if (c.k < k1) {
      const int i = order[c.k];
      if (i >= 0 && i < g.Ho) c.i = i, c.nt = min(max(ntap[i], 0), g.rw_pitch), c.r0 = row0[i];
    }
  };
  int tag0 = 0, tag1 = 0, old = 0;          // the two kept inner: their global rows, which one goes next
  bool v0 = false, v1 = false;
  double in0 = 0.0, in1 = 0.0;
  // the first position from c on whose row is not kept; false: none before k1
  auto next_miss = [&](Cur &c) {
    while (c.k < k1) {
      if (c.t < c.nt) {
        const int h = c.r0 + c.t;
        if (!(v0 && h == tag0) && !(v1 && h == tag1)) return true;
        ++c.t;
      } else {
        ++c.k, c.t = 0;
        window(c);
      }
    }
    return false;
  };
  auto row_ok = [&](int h) { return load_ok && h >= g.src_r0 && h < g.src_r0 + g.Hs; };
  auto spans_of = [&](int h) {
    const float *row = chan + (size_t)(h - g.src_r0) * g.Ws;
    s.mis0 = (int)(((uintptr_t)(row + s.l0) >> 2) & 3);
    s.nq0 = (s.mis0 + s.n0 + 3) >> 2;
    s.mis1 = (int)(((uintptr_t)row >> 2) & 3);
    s.nq1 = s.n1 > 0 ? (s.mis1 + s.n1 + 3) >> 2 : 0;
    return row;
  };

  float4 r[MAXQ];
  Cur L;                                    // the look-ahead: the position whose row LDS holds (or is about to)
  L.k = k0, L.t = 0;
  window(L);
  if (next_miss(L) && row_ok(L.r0 + L.t)) {
    const float *row = spans_of(L.r0 + L.t);
    issue_row(row, s, r);
    commit_row(lds, s, r);
  }
  __syncthreads();                          // the row and the column weights are in LDS

  for (int k = k0; k < k1; ++k) {
    Cur M;
    M.k = k, M.t = 0;
    window(M);
    double acc = 0.0;
    for (int t = 0; t < M.nt; ++t) {
      const int h = M.r0 + t;
      if (!(v0 && h == tag0) && !(v1 && h == tag1)) {
        // a miss: L stands here and LDS holds row h.  Keep its inner in place of the older one ...
        const bool h_ok = row_ok(h);
        const int slot = old;
        old ^= 1;
        if (slot == 0) tag0 = h, v0 = true; else tag1 = h, v1 = true;
        // ... and put the next row to stage in flight before this one is reduced
        ++L.t;
        const bool more = next_miss(L);
        const bool nh_ok = more && row_ok(L.r0 + L.t);
        Span sn = s;
        if (nh_ok) {
          const float *row = spans_of(L.r0 + L.t);
          sn = s;
          issue_row(row, sn, r);
        }
        double in = 0.0;
        if (h_ok) {
          if (col_ok)
            for (int u = 0; u < ct; ++u) in = in + cwl[u * g.tile_cols + j] * (double)lds[lds_at(off + u)];
        } else {
          in = __builtin_nan("");           // a row outside the source is not read
        }
        if (slot == 0) in0 = in; else in1 = in;
        if (more) {
          __syncthreads();                  // every thread has read the row in LDS
          if (nh_ok) commit_row(lds, sn, r);
          __syncthreads();
        }
      }
      const double in = (v0 && h == tag0) ? in0 : in1;
      acc = acc + rw[(size_t)M.i * g.rw_pitch + t] * in;
    }
    if (owner && M.i >= 0) out[(size_t)M.i * g.Wo] = (col_ok && M.nt > 0) ? (float)acc : __builtin_nanf("");
  }
}

}  // namespace

extern "C" int cra5_regrid_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W, int Ho,
                               int Wo, const int *row0, const int *ntap, const double *rw, int rw_pitch, const int *order,
                               const int *col0, const int *ctap, const double *cw, int cw_pitch, const int *tiles,
                               int n_tiles, int tile_cols, int max_span, const int *chan_map, int C_out, float *dst,
                               void *stream) {
  if (!src || !dst || !row0 || !ntap || !rw || !order || !col0 || !ctap || !cw || !tiles) return CRA5_ERR_ARG;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row0 & 3) || ((uintptr_t)ntap & 3) ||
      ((uintptr_t)rw & 7) || ((uintptr_t)order & 3) || ((uintptr_t)col0 & 3) || ((uintptr_t)ctap & 3) ||
      ((uintptr_t)cw & 7) || ((uintptr_t)tiles & 3) || ((uintptr_t)chan_map & 3))
    return CRA5_ERR_ARG;
  if (C_src <= 0 || C_out <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || rw_pitch <= 0 ||
      cw_pitch <= 0 || n_tiles <= 0 || tile_cols <= 0 || max_span <= 0)
    return CRA5_ERR_ARG;
  if (!chan_map && C_out > C_src) return CRA5_ERR_ARG;
  // the source box lies in the grid; a box as wide as the grid is the whole circle from column 0
  if (src_r0 < 0 || Hs > H - src_r0 || src_c0 < 0 || src_c0 >= W || Ws > W) return CRA5_ERR_ARG;
  if (Ws == W && src_c0 != 0) return CRA5_ERR_ARG;
  if (rw_pitch > H || cw_pitch > CTAP_MAX || cw_pitch > W) return CRA5_ERR_ARG;
  if (tile_cols > THREADS || (long long)tile_cols * cw_pitch > CW_MAX_DOUBLES || n_tiles > Wo) return CRA5_ERR_ARG;
  if (max_span > SPAN_MAX || max_span > 2LL * W) return CRA5_ERR_ARG;

  Geo g;
  g.Hs = Hs, g.Ws = Ws, g.src_r0 = src_r0, g.src_c0 = src_c0, g.W = W, g.whole = Ws == W ? 1 : 0;
  g.Ho = Ho, g.Wo = Wo, g.rw_pitch = rw_pitch, g.cw_pitch = cw_pitch;
  g.n_tiles = n_tiles, g.tile_cols = tile_cols, g.max_span = max_span;
  // enough blocks to fill the chip several times over; a longer run of rows re-stages fewer shared source rows
  const long long per_row = (long long)C_out * n_tiles;
  long long chunks = (4096 + per_row - 1) / per_row;
  if (chunks > Ho) chunks = Ho;
  if (chunks < 1) chunks = 1;
  g.rows_per_block = (int)((Ho + chunks - 1) / chunks);
  g.n_chunks = (Ho + g.rows_per_block - 1) / g.rows_per_block;
  const long long blocks = per_row * g.n_chunks;
  if (blocks > 0x7fffffffLL) return CRA5_ERR_ARG;
  const size_t lds_bytes = (size_t)cw_pitch * tile_cols * sizeof(double) +
                           (size_t)(max_span + (max_span >> 5) + 1) * sizeof(float);
  hipLaunchKernelGGL(regrid_kernel, dim3((unsigned)blocks), dim3(THREADS), lds_bytes, (hipStream_t)stream, src, row0, ntap,
                     rw, order, col0, ctap, cw, tiles, chan_map, C_src, dst, g);
  return (int)hipGetLastError();
}
