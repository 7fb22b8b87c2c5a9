// Exact Euclidean distance transform of an occupancy grid: for every cell the squared distance, in cells, to the nearest
// occupied cell and (optionally) which cell that is.  What a clearance margin for the grid-search seeds (grid_search.hip)
// is decided on: a cell of the inflated image is a wall iff dist2 <= k.
//
// Everything is integer arithmetic on at most 4096 x 4096 cells, so a squared distance stays below 2^25 and the result
// is the same whatever the schedule; there are no atomics and no floating point.
//
// The transform is separable.  With g(row, col') = the occupied row of column col' nearest to `row` (the SMALLER row when
// the one above and the one below are equally far),
//   dist2(row, col) = min over col' of (col - col')^2 + (row - g(row, col'))^2.
// The tie rule of the result -- among equidistant occupied cells the smallest flat index row * cols + col, i.e. the
// smallest row and then the smallest column -- is kept by taking the minimum of the triple (distance, g, col'): a column
// offers its nearest cell only, another cell of the same column is at least as far, and at equal distance the column pass
// has already kept the smaller row.
#include "common.h"

#include <limits.h>

namespace nfopp {

constexpr int EDT_MAX_SIDE = 4096;
constexpr long long EDT_MAX_CELLS = 1LL << 24;   // the limit of nfopp_grid_to_points
constexpr int EDT_COLS_PER_BLOCK = 64;           // one wave reads 64 consecutive bytes of a row
constexpr int EDT_SEGMENTS = 16;                 // row segments of a column, one thread each
constexpr int EDT_ROW_THREADS = 256;

struct EdtArgs {
  const unsigned char* occ;   // [rows, cols]
  int rows, cols, border;
  int* g;                     // workspace [rows, cols]: nearest occupied row of the column, -1 = the column is empty
  int* dist2;                 // [rows, cols]
  int* nearest;               // [rows, cols] or null
};

// ---- column pass ------------------------------------------------------------------------------------------------------
// A workgroup takes 64 adjacent columns, thread (x, y) the y-th of 16 row segments of column x; adjacent lanes read
// adjacent bytes.  Each thread first finds the first and last occupied row of its segment; from those every thread knows
// the last occupied row above its segment and the first one below it, walks down its segment writing the nearest occupied
// row at or above each cell, then up again comparing it with the nearest at or below.
__global__ __launch_bounds__(EDT_COLS_PER_BLOCK * EDT_SEGMENTS) void edt_column_kernel(const EdtArgs a) {
  __shared__ int seg_first[EDT_SEGMENTS][EDT_COLS_PER_BLOCK];
  __shared__ int seg_last[EDT_SEGMENTS][EDT_COLS_PER_BLOCK];
  const int rows = a.rows, cols = a.cols;
  const int x = threadIdx.x, y = threadIdx.y;
  const int c = blockIdx.x * EDT_COLS_PER_BLOCK + x;
  const int seg_len = (rows + EDT_SEGMENTS - 1) / EDT_SEGMENTS;
  const int r0 = min(y * seg_len, rows), r1 = min(r0 + seg_len, rows);
  const bool live = c < cols;
  int first = -1, last = -1;
  if (live) {
    const unsigned char* occ = a.occ + c;
    for (int r = r0; r < r1; ++r)
      if (occ[(long long)r * cols] != 0) {
        if (first < 0) first = r;
        last = r;
      }
  }
  seg_first[y][x] = first;
  seg_last[y][x] = last;
  __syncthreads();
  if (!live) return;
  int up = -1, dn = -1;
  for (int s = 0; s < y; ++s) {
    const int v = seg_last[s][x];
    if (v >= 0) up = v;
  }
  for (int s = EDT_SEGMENTS - 1; s > y; --s) {
    const int v = seg_first[s][x];
    if (v >= 0) dn = v;
  }
  const unsigned char* occ = a.occ + c;
  int* g = a.g + c;
  for (int r = r0; r < r1; ++r) {
    if (occ[(long long)r * cols] != 0) up = r;
    g[(long long)r * cols] = up;
  }
  for (int r = r1 - 1; r >= r0; --r) {
    const int above = g[(long long)r * cols];   // this thread's own store
    if (above == r) dn = r;
    int pick = above;
    // strictly nearer below; on a tie the row above (the smaller flat index) stays
    if (dn >= 0 && (above < 0 || dn - r < r - above)) pick = dn;
    g[(long long)r * cols] = pick;
  }
}

// ---- row pass ---------------------------------------------------------------------------------------------------------
// A workgroup holds g of one row in LDS (of 256 / cols rows when the grid is narrower than the workgroup) and every thread
// scans outward from its cell: offsets k = 0, 1, 2, ... to both sides, until k^2 alone exceeds the best distance so far
// (at k^2 == best a column with g on this very row still ties, and the tie may have the smaller index).  Lanes of a wave
// sit on adjacent cells and step k together, so their LDS reads fall on adjacent words.
// The candidates are ordered by one 64-bit key: distance (< 2^25) above the row g (12 bits) above the column (12 bits).
__device__ __forceinline__ unsigned long long edt_key(int dcol, int row, int grow, int col) {
  const int drow = row - grow;
  const unsigned int d = (unsigned int)(dcol * dcol + drow * drow);
  return ((unsigned long long)d << 24) | ((unsigned long long)(unsigned int)grow << 12) | (unsigned int)col;
}

__global__ __launch_bounds__(EDT_ROW_THREADS) void edt_row_kernel(const EdtArgs a) {
  __shared__ int g_lds[EDT_MAX_SIDE];
  const int rows = a.rows, cols = a.cols;
  const int rows_here = cols >= EDT_ROW_THREADS ? 1 : EDT_ROW_THREADS / cols;
  const int row0 = blockIdx.x * rows_here;
  const int n_rows = min(rows_here, rows - row0);
  const int items = n_rows * cols;   // <= 4096: one row of at most 4096 cells, or rows_here * cols <= 256
  const int* g = a.g + (long long)row0 * cols;
  for (int i = threadIdx.x; i < items; i += EDT_ROW_THREADS) g_lds[i] = g[i];
  __syncthreads();
  constexpr unsigned long long NONE = ~0ull;
  for (int i = threadIdx.x; i < items; i += EDT_ROW_THREADS) {
    const int lr = i / cols, c = i - lr * cols;
    const int row = row0 + lr;
    const int* gr = g_lds + lr * cols;
    unsigned long long best = NONE;
    unsigned int best_d = 0xffffffffu;
    const int reach = max(c, cols - 1 - c);
    for (int k = 0; k <= reach && (unsigned int)(k * k) <= best_d; ++k) {
      const int cl = c - k, cr = c + k;
      if (cl >= 0) {
        const int gl = gr[cl];
        if (gl >= 0) {
          const unsigned long long key = edt_key(k, row, gl, cl);
          if (key < best) best = key;
        }
      }
      if (cr < cols && k > 0) {
        const int gv = gr[cr];
        if (gv >= 0) {
          const unsigned long long key = edt_key(k, row, gv, cr);
          if (key < best) best = key;
        }
      }
      best_d = (unsigned int)(best >> 24);   // NONE gives 2^40 - 1 truncated to 0xffffffff: still "no bound"
    }
    int d = INT_MAX, idx = -1;
    if (best != NONE) {
      d = (int)(best >> 24);
      idx = (int)((best >> 12) & 0xfffu) * cols + (int)(best & 0xfffu);
    }
    if (a.border) {
      // cells outside the matrix count as occupied: the nearest of them is b cells away, straight across the nearest side
      const int b = min(min(row + 1, rows - row), min(c + 1, cols - c));
      d = min(d, b * b);
    }
    const long long o = (long long)row * cols + c;
    a.dist2[o] = d;
    if (a.nearest) a.nearest[o] = idx;
  }
}

static bool edt_shape_ok(int rows, int cols) {
  return rows >= 1 && cols >= 1 && rows <= EDT_MAX_SIDE && cols <= EDT_MAX_SIDE && (long long)rows * cols <= EDT_MAX_CELLS;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_grid_edt_workspace_bytes(int32_t rows, int32_t cols) {
  if (!edt_shape_ok(rows, cols)) return 0;
  return (size_t)rows * (size_t)cols * sizeof(int32_t);
}

extern "C" int nfopp_grid_edt(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t border, int32_t* dist2_dev,
                              int32_t* nearest_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1, "grid must have at least one row and one column");
  NFOPP_REQUIRE(rows <= EDT_MAX_SIDE && cols <= EDT_MAX_SIDE, "grid must be at most %d cells a side", EDT_MAX_SIDE);
  NFOPP_REQUIRE((long long)rows * cols <= EDT_MAX_CELLS, "grid has more than 2^24 cells");
  NFOPP_REQUIRE(occupancy_dev && dist2_dev, "null device pointer");
  const size_t need = nfopp_grid_edt_workspace_bytes(rows, cols);
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small: nfopp_grid_edt_workspace_bytes gives %zu", need);
  NFOPP_REQUIRE(((uintptr_t)workspace_dev & 3) == 0, "workspace must be 4-byte aligned");
  EdtArgs a;
  a.occ = occupancy_dev; a.rows = rows; a.cols = cols; a.border = border ? 1 : 0;
  a.g = reinterpret_cast<int*>(workspace_dev); a.dist2 = dist2_dev; a.nearest = nearest_dev;
  const unsigned col_blocks = (unsigned)((cols + EDT_COLS_PER_BLOCK - 1) / EDT_COLS_PER_BLOCK);
  hipLaunchKernelGGL(edt_column_kernel, dim3(col_blocks), dim3(EDT_COLS_PER_BLOCK, EDT_SEGMENTS), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  const int rows_here = cols >= EDT_ROW_THREADS ? 1 : EDT_ROW_THREADS / cols;
  const unsigned row_blocks = (unsigned)((rows + rows_here - 1) / rows_here);
  hipLaunchKernelGGL(edt_row_kernel, dim3(row_blocks), dim3(EDT_ROW_THREADS), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
