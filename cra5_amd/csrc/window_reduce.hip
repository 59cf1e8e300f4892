// The windowed reduction behind coarsen= and regrid= ("Coarsening" and "Regridding"): a decoded frame
// through per-row and per-column windows, one streaming pass.
//
//   inner(h, j)  = sum over the columns of output column j's window, west to east, of weight * (double)x[h][column mod W]
//   out[c][i][j] = (float) sum over t = 0 .. ntap[i] - 1, north to south, of rw[i][t] * inner(row0[i] + t, j)
//
// in float64, every sum starting from 0, every product and every add rounded on its own (contraction off).  inner depends
// on the GLOBAL (h, j) only and a row sum on the output row only: results are bit-identical from run to run, and a
// region's or a sub-grid's result is the sub-block of the whole one's.
//
//   cra5_coarsen_f32 (cra5_amd/subset.py coarsen_plan): output column j is global column (col0 + j * k_lon) mod W, its
//     window the columns - k_lon / 2 .. + k_lon / 2 around it, weight 1/2 on the two edge columns of an even k_lon, 1
//     elsewhere (1/2 * x is exact: one add per column).  Tiles of <= 256 output columns by arithmetic, no weights in LDS.
//   cra5_regrid_f32 (cra5_amd/regrid.py Grid.plan: bilinear, first-order conservative): window col0[j] .. + ctap[j] - 1
//     with weights cw[j][.], one product and one add per column.  The tiles come from the host (regrid.tile_table):
//     consecutive target columns - monotone, so one eastward span - that fit the budget.  The weights sit in LDS as
//     [tap][column] (conflict-free), loaded once per block - they never join the per-row HBM stream.
//
// Staging, shared by both.  One block = one channel x one column tile x a run of output rows, walked north to south.  Per
// source row the block stages the tile's span - at most two contiguous pieces when it crosses the source's east edge - in
// LDS with 16-byte loads (the pieces' first / last partial quads go element by element: any 4-byte aligned base works),
// and the loads of the NEXT row to stage are issued before the current row is reduced, so they fly under the LDS reads and
// the fp64 arithmetic.  Each thread owns one output column and keeps the row sum in a register; a column two windows
// share is read from LDS twice, from HBM once.  The launchers split the output rows into runs so that a launch has
// >= 4096 blocks; only at the start of a run is a source row that two runs share staged a second time.
//
// The walks.  Coarsening's windows are regular - consecutive output rows share at most their edge row (even k_lat) -, so
// its kernel carries ONE inner to the next output row.  The table-driven kernel walks through `order` (the target rows
// sorted north to south; row order[k] is WRITTEN, so a south-to-north target comes back in the caller's order) and keeps
// the inner of the two most recently staged source rows in registers, tagged by global row: bilinear at any ratio and
// conservative windows that share at most their edge row stage every source row once per block.  It computes
// coarsening's cells with the same bits, but measured 6-7 % slower than the one-inner walk at k_lon = 2 and 24
// (profiles/window_reduce_ab.txt): coarsening keeps its own.
//
// Bank conflicts.  Index i of the staged row lives at dword i + i / 32.  By the bank rule of a 4-byte LDS read (bank =
// dword mod 32, conflicts counted inside each 32-lane half) a lane stride of k_lon dwords is gcd(k_lon, 32)-way
// conflicted unpadded: 2-way at k_lon = 2, 6, 10, 4-way at 4 and 12, 8-way at 8 and 24, 32-way at 32, none at an odd
// k_lon.  With the padding every k_lon from 2 to 32 is at most 2-way, on some of the k_lon + 1 reads (an odd k_lon pays
// for it: none -> 2-way).  The degree is computed from the rule, not measured with a counter.
//
// Limits the launchers enforce.  The loads in flight hold 256 x 8 quads, and each of two pieces may open and close a
// partial one: a staged span holds at most 8176 floats (coarsening: k_lon <= 8175).  A table-driven launch keeps the
// padded row inside 32 KB - 7936 floats, its piece past the east edge at most one row (W) - beside 32 KB of column
// weights: ctap <= cw_pitch <= 64 (cw_pitch x tile columns x 8 bytes; 64 taps leave 64 columns per tile - a 5.625 deg
// target on the 0.25 deg grid takes 23 or 24), ntap <= rw_pitch <= H (rows are streamed, a window cannot hold more rows
// than the grid).  The tables live on the device, so the kernels check every entry before use: a row or a column window
// outside the source, a tile span outside the source or the budget, an empty row window or a channel outside the source
// is never read - those outputs become NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cra5_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAXQ = 8;                              // 16-byte loads in flight per thread and row
constexpr int STAGE_MAX = THREADS * MAXQ * 4 - 16;   // floats the loads in flight hold: two pieces, a partial quad at each end
constexpr int SPAN_MAX = 7936;                       // table-driven: (n + n / 32 + 1) * 4 <= 32 KB
constexpr int CW_MAX_DOUBLES = 4096;                 // cw_pitch * tile columns: 32 KB
constexpr int CTAP_MAX = 64;

struct Geo {
  int Hs, Ws, src_r0, src_c0, W;          // source [.][Hs][Ws], its first global row / column
  int k_lat, Ho, k_lon, Wo, col0;         // coarsening's output progression: column j = (col0 + j * k_lon) mod W
  int rw_pitch, tile_cols, n_tiles, rows_per_block, n_chunks;
  int whole, cw_pitch, max_span;          // table-driven; whole: Ws == W
};

__device__ __forceinline__ int lds_at(int i) { return i + (i >> 5); }

// The staged span of one source row: piece 0 = n0 floats from local column l0, piece 1 = n1 floats from local column 0
// (the part past the east edge of a whole-circle source).  Quad q of a piece covers elements 4 q - mis .. + 3 of it,
// mis = the piece's first element's offset inside its 16-byte line.
struct Span {
  int l0, n0, n1, mis0, nq0, mis1, nq1;
};

// The quads of span s (l0, n0, n1 set) on the source row at `row`.
__device__ __forceinline__ void align_span(Span &s, const float *row) {
  s.mis0 = (int)(((uintptr_t)(row + s.l0) >> 2) & 3);
  s.nq0 = (s.mis0 + s.n0 + 3) >> 2;
  s.mis1 = (int)(((uintptr_t)row >> 2) & 3);
  s.nq1 = s.n1 > 0 ? (s.mis1 + s.n1 + 3) >> 2 : 0;
}

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
    align_span(s, row);
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

// A position of the table-driven walk: tap t of the window of target row i = order[k].
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
    align_span(s, row);
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

// What both entry points check alike - the pointers, the sizes, the channel count, the source box inside the grid - and
// the geometry both kernels read.
bool common_args(Geo &g, const float *src, const float *dst, const int *row0, const int *ntap, const double *rw,
                 const int *chan_map, int C_src, int C_out, int Hs, int Ws, int src_r0, int src_c0, int H, int W, int Ho,
                 int Wo, int rw_pitch) {
  if (!src || !dst || !row0 || !ntap || !rw) return false;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row0 & 3) || ((uintptr_t)ntap & 3) ||
      ((uintptr_t)rw & 7) || ((uintptr_t)chan_map & 3))
    return false;
  if (C_src <= 0 || C_out <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || rw_pitch <= 0)
    return false;
  if (!chan_map && C_out > C_src) return false;
  if (src_r0 < 0 || Hs > H - src_r0 || src_c0 < 0 || src_c0 >= W || Ws > W) return false;
  g = Geo();
  g.Hs = Hs, g.Ws = Ws, g.src_r0 = src_r0, g.src_c0 = src_c0, g.W = W, g.whole = Ws == W ? 1 : 0;
  g.Ho = Ho, g.Wo = Wo, g.rw_pitch = rw_pitch;
  return true;
}

// Rows per block, from g.n_tiles and g.Ho: enough blocks to fill the chip several times over; a longer run of rows
// re-stages fewer shared source rows.  -> the number of blocks, 0: more than a launch holds.
long long chunk_rows(Geo &g, int C_out) {
  const long long per_row = (long long)C_out * g.n_tiles;
  long long chunks = (4096 + per_row - 1) / per_row;
  if (chunks > g.Ho) chunks = g.Ho;
  if (chunks < 1) chunks = 1;
  g.rows_per_block = (int)((g.Ho + chunks - 1) / chunks);
  g.n_chunks = (g.Ho + g.rows_per_block - 1) / g.rows_per_block;
  const long long blocks = per_row * g.n_chunks;
  return blocks > 0x7fffffffLL ? 0 : blocks;
}

size_t row_lds_bytes(int n_span) { return (size_t)(n_span + (n_span >> 5) + 1) * sizeof(float); }

}  // namespace

extern "C" int cra5_coarsen_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W,
                                int whole_circle, int out_r0, int k_lat, int Ho, int out_c0, int k_lon, int Wo,
                                const int *row0, const int *ntap, const double *rw, int rw_pitch, const int *chan_map,
                                int C_out, float *dst, void *stream) {
  Geo g;
  if (!common_args(g, src, dst, row0, ntap, rw, chan_map, C_src, C_out, Hs, Ws, src_r0, src_c0, H, W, Ho, Wo, rw_pitch))
    return CRA5_ERR_ARG;
  if (k_lat <= 0 || k_lon <= 0) return CRA5_ERR_ARG;
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
  if ((long long)k_lon + 1 > STAGE_MAX) return CRA5_ERR_ARG;

  g.k_lat = k_lat, g.k_lon = k_lon, g.col0 = out_c0;
  int tc = (STAGE_MAX - 2 * half - 1) / k_lon + 1;      // (tc - 1) * k_lon + 2 * half + 1 <= STAGE_MAX
  if (tc > THREADS) tc = THREADS;
  if (tc > Wo) tc = Wo;
  g.tile_cols = tc;
  g.n_tiles = (Wo + tc - 1) / tc;
  const long long blocks = chunk_rows(g, C_out);
  if (!blocks) return CRA5_ERR_ARG;
  hipLaunchKernelGGL(coarsen_kernel, dim3((unsigned)blocks), dim3(THREADS), row_lds_bytes((tc - 1) * k_lon + 2 * half + 1),
                     (hipStream_t)stream, src, row0, ntap, rw, chan_map, C_src, dst, g);
  return (int)hipGetLastError();
}

extern "C" int cra5_regrid_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W, int Ho,
                               int Wo, const int *row0, const int *ntap, const double *rw, int rw_pitch, const int *order,
                               const int *col0, const int *ctap, const double *cw, int cw_pitch, const int *tiles,
                               int n_tiles, int tile_cols, int max_span, const int *chan_map, int C_out, float *dst,
                               void *stream) {
  Geo g;
  if (!common_args(g, src, dst, row0, ntap, rw, chan_map, C_src, C_out, Hs, Ws, src_r0, src_c0, H, W, Ho, Wo, rw_pitch))
    return CRA5_ERR_ARG;
  if (!order || !col0 || !ctap || !cw || !tiles) return CRA5_ERR_ARG;
  if (((uintptr_t)order & 3) || ((uintptr_t)col0 & 3) || ((uintptr_t)ctap & 3) || ((uintptr_t)cw & 7) ||
      ((uintptr_t)tiles & 3))
    return CRA5_ERR_ARG;
  if (cw_pitch <= 0 || n_tiles <= 0 || tile_cols <= 0 || max_span <= 0) return CRA5_ERR_ARG;
  // a box as wide as the grid is the whole circle from column 0
  if (Ws == W && src_c0 != 0) return CRA5_ERR_ARG;
  if (rw_pitch > H || cw_pitch > CTAP_MAX || cw_pitch > W) return CRA5_ERR_ARG;
  if (tile_cols > THREADS || (long long)tile_cols * cw_pitch > CW_MAX_DOUBLES || n_tiles > Wo) return CRA5_ERR_ARG;
  if (max_span > SPAN_MAX || max_span > 2LL * W) return CRA5_ERR_ARG;

  g.cw_pitch = cw_pitch, g.n_tiles = n_tiles, g.tile_cols = tile_cols, g.max_span = max_span;
  const long long blocks = chunk_rows(g, C_out);
  if (!blocks) return CRA5_ERR_ARG;
  hipLaunchKernelGGL(regrid_kernel, dim3((unsigned)blocks), dim3(THREADS),
                     (size_t)cw_pitch * tile_cols * sizeof(double) + row_lds_bytes(max_span), (hipStream_t)stream, src, row0,
                     ntap, rw, order, col0, ctap, cw, tiles, chan_map, C_src, dst, g);
  return (int)hipGetLastError();
}
