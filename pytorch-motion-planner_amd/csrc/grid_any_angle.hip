// Any-angle shortening of grid-search cell paths by exact line of sight: B cell paths on one shared grid -> per path the
// anchors (indices into the path) between which the cells are skipped, and the polyline through the anchors refilled at
// the cell path's own density, ready for the spline stage (nfopp_grid_seed_polylines, grid_search.hip).
//
// The rule is this library's own and is stated in include/nfopp_hip.h.  In short: cell A sees cell B iff no blocked cell
// other than A and B has an open interior met by the segment between the two centres; the cells are visited by an integer
// merge of the segment's column and row crossings; a cell is blocked iff dist2 <= the problem's threshold (dist2 from
// nfopp_grid_edt, border 0); the next anchor is the FARTHEST cell within `lookahead` that the current one sees.
//
// Everything that decides an anchor is int32 arithmetic, so the result does not depend on the schedule; the points are
// float64 with every operation rounded on its own, stored fp32.
#include "common.h"
#include "grid_frame.h"

namespace nfopp {

constexpr int AA_WAVES = 4;                 // problems of a workgroup, one wavefront each
constexpr int AA_THREADS = 64 * AA_WAVES;
constexpr int AA_MAX_SIDE = 4096;           // the limits of nfopp_grid_edt, whose output is read here
constexpr long long AA_MAX_CELLS = 1LL << 24;

struct ShortenArgs {
  const int* dist2;         // [rows, cols]
  int rows, cols;
  const int* cells;         // [B, max_len, 2] (row, col)
  const int* count; const int* status;
  const int* cells2;        // [B] or null
  long long batch;
  int max_len, lookahead;
  int* anchor;              // [B, max_len]
  int* anchor_count;
  double ox, oy, res;
  int max_points;
  float* points;            // [B, max_points, 2] or null
  int* point_count;
};

// The traversal.  Column crossing i = 1..ac of the segment lies at parameter (2i - 1) / (2 ac), row crossing j = 1..ar at
// (2j - 1) / (2 ar); they are merged by comparing (2i - 1) ar with (2j - 1) ac (at most 2 * 4096 * 4096 = 2^25).  Equal
// means the segment passes through a lattice corner: both steps are taken at once and only the diagonal cell is visited.
// The walk ends at its first blocked cell; B itself is reached but not tested, A never visited.  Both cells lie inside the
// grid, so every cell between them does.
__device__ __forceinline__ bool sees(const int* __restrict__ dist2, int cols, int thr, int2 A, int2 B) {
  const int dr = B.x - A.x, dc = B.y - A.y;
  const int ar = abs(dr), ac = abs(dc);
  const int sr = dr < 0 ? -1 : 1, sc = dc < 0 ? -1 : 1;
  int i = 1, j = 1, r = A.x, c = A.y;
  while (i <= ac || j <= ar) {
    const bool col_left = i <= ac, row_left = j <= ar;
    const int ck = (2 * i - 1) * ar, rk = (2 * j - 1) * ac;
    const bool step_col = col_left && (!row_left || ck <= rk);
    const bool step_row = row_left && (!col_left || rk <= ck);
    if (step_col) { c += sc; ++i; }
    if (step_row) { r += sr; ++j; }
    if (i > ac && j > ar) break;
    if (dist2[r * cols + c] <= thr) return false;
  }
  return true;
}

// the fractional cell coordinates below are float64 with every operation rounded on its own; their centres in metres are
// grid_cell_centre's (grid_frame.h), the seeding stage's too
#pragma clang fp contract(off)

__global__ __launch_bounds__(AA_THREADS) void shorten_kernel(const ShortenArgs a) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * AA_WAVES + (threadIdx.x >> 6);
  if (p >= a.batch) return;   // whole wavefronts leave: no lane of a live one is missing below
  const int n = __builtin_amdgcn_readfirstlane(a.count[p]);
  bool ok = a.status[p] == 0 && n >= 1 && n <= a.max_len;
  const int2* cells = reinterpret_cast<const int2*>(a.cells) + p * a.max_len;
  if (ok) {
    // a caller-made list may name cells outside the grid: such a row is refused like a failed search, so that no walk
    // below leaves dist2
    bool outside = false;
    for (int k = lane; k < n; k += 64) {
      const int2 rc = cells[k];
      outside |= rc.x < 0 || rc.x >= a.rows || rc.y < 0 || rc.y >= a.cols;
    }
    ok = !__any(outside);
  }
  if (!ok) {
    if (lane == 0) { a.anchor_count[p] = 0; a.point_count[p] = 0; }
    return;
  }
  const int thr = a.cells2 ? __builtin_amdgcn_readfirstlane(a.cells2[p]) : 0;
  const int look = min(a.lookahead, n);
  int* anchor = a.anchor + p * a.max_len;
  float* pts = a.points ? a.points + p * a.max_points * 2 : nullptr;
  int at = 0, n_anchors = 1;
  long long n_points = 0;   // the running sum of the segments' m: where the next segment's points go
  if (lane == 0) anchor[0] = 0;
  while (at < n - 1) {
    const int2 A = cells[at];
    const int last = min(at + look, n - 1);
    // rounds of 64 candidates, farthest first: lane l takes j = hi - l and the lowest set bit of the ballot is the farthest
    // cell of the round that A sees.  Visibility along a path is not monotone, so a round without one says nothing about
    // the next.
    int next = -1;
    for (int hi = last; hi > at && next < 0; hi -= 64) {
      const int j = hi - lane;
      bool v = false;
      if (j > at) v = sees(a.dist2, a.cols, thr, A, cells[j]);
      const unsigned long long seen = __ballot(v);
      if (seen) next = hi - (__ffsll((long long)seen) - 1);
    }
    if (next < 0) next = at + 1;   // not 8-connected (consecutive cells of a traced path always see each other)
    next = __builtin_amdgcn_readfirstlane(next);
    if (lane == 0) anchor[n_anchors] = next;
    ++n_anchors;
    const int2 Bc = cells[next];
    const int dr = Bc.x - A.x, dc = Bc.y - A.y;
    const int m = max(abs(dr), abs(dc));
    if (pts) {
      for (int t = lane; t < m && n_points + t < a.max_points; t += 64) {
        const double ur = (double)A.x + (double)(dr * t) / (double)m;
        const double uc = (double)A.y + (double)(dc * t) / (double)m;
        float* q = pts + (n_points + t) * 2;
        q[0] = grid_cell_centre(uc, a.res, a.ox);
        q[1] = grid_cell_centre(ur, a.res, a.oy);
      }
    }
    n_points += m;
    at = next;
  }
  if (lane == 0) {
    if (pts && n_points < a.max_points) {
      const int2 E = cells[n - 1];
      pts[n_points * 2] = grid_cell_centre((double)E.y, a.res, a.ox);
      pts[n_points * 2 + 1] = grid_cell_centre((double)E.x, a.res, a.oy);
    }
    a.anchor_count[p] = n_anchors;
    a.point_count[p] = (int)min(n_points + 1, (long long)INT32_MAX);
  }
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_grid_shorten_paths(const int32_t* dist2_dev, int32_t rows, int32_t cols, const int32_t* cells_dev,
                                        const int32_t* count_dev, const int32_t* status_dev, const int32_t* cells2_dev,
                                        int64_t batch, int32_t max_len, int32_t lookahead, int32_t* anchor_dev,
                                        int32_t* anchor_count_dev, double origin_x, double origin_y, double resolution,
                                        int32_t max_points, float* points_dev, int32_t* point_count_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1, "grid must have at least one row and one column");
  NFOPP_REQUIRE(rows <= AA_MAX_SIDE && cols <= AA_MAX_SIDE && (long long)rows * cols <= AA_MAX_CELLS,
                "grid must be at most %d cells a side, as for nfopp_grid_edt", AA_MAX_SIDE);
  NFOPP_REQUIRE(lookahead >= 1, "lookahead must be at least 1");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && max_len >= 0 && max_points >= 0, "bad sizes");
  NFOPP_REQUIRE(max_len <= (1 << 21) + 1, "path buffer longer than any path of a supported grid");
  NFOPP_REQUIRE(resolution > 0.0, "bad resolution");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(dist2_dev && count_dev && status_dev && anchor_count_dev && point_count_dev, "null device pointer");
  NFOPP_REQUIRE((cells_dev && anchor_dev) || max_len == 0, "null device pointer");
  ShortenArgs a;
  a.dist2 = dist2_dev; a.rows = rows; a.cols = cols; a.cells = cells_dev; a.count = count_dev; a.status = status_dev;
  a.cells2 = cells2_dev; a.batch = batch; a.max_len = max_len; a.lookahead = lookahead; a.anchor = anchor_dev;
  a.anchor_count = anchor_count_dev; a.ox = origin_x; a.oy = origin_y; a.res = resolution; a.max_points = max_points;
  a.points = max_points > 0 ? points_dev : nullptr; a.point_count = point_count_dev;
  hipLaunchKernelGGL(shorten_kernel, dim3((unsigned)((batch + AA_WAVES - 1) / AA_WAVES)), dim3(AA_THREADS), 0,
                     (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
