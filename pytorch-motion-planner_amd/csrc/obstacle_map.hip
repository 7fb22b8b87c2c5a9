// The obstacle update of the receding-horizon loop, on the device: occupancy grid -> point cloud, and the uniform cell index
// the ground-truth checkers of csrc/sampling.hip search (nfopp_check_collision_circle_cells / _rectangle_cells).
//
// Replaces (reference, host numpy, once per sensor message):
//   * `GridMap.as_point_cloud` nfop/ros/grid_map.py:14-20 and the unpacking of `from_ros_occupancy_grid` :31-40
//   * the index `DeviceCircleChecker` used to build on the host (np.argsort(kind="stable") + np.searchsorted)
// Everything here is integer counting plus per-element arithmetic: no atomics, every sum in a fixed order, so both
// results are bit-identical from run to run.  All kernels are latency-bound helpers that run at map rate.
#include "block_collectives.h"
#include "common.h"
#include "point_cloud.h"

namespace nfopp {

constexpr int OM_THREADS = 256;             // 4 waves of 64
constexpr int OM_WAVES = OM_THREADS / 64;

// ---- grid -> point cloud -----------------------------------------------------------------------------------------
// Order-preserving compaction in three launches: (1) occupied cells per chunk of GP_CHUNK cells (ballot + popcount),
// (2) exclusive scan of the chunk counts by one workgroup, GP_SCAN_PASS counts per pass with a carry, (3) the predicate
// again, each point stored at chunk offset + rank inside the chunk.
constexpr int GP_TILES = 8;
constexpr int GP_CHUNK = OM_THREADS * GP_TILES;   // 2048 cells per workgroup
constexpr int GP_SCAN_PASS = OM_THREADS;          // chunk counts one scan pass takes
constexpr long long GP_MAX_CELLS = 1ll << 24;

struct GridArgs {
  const void* grid; int cells, cols; float threshold;
  double resolution, half, ox, oy, c, s;
  int n_chunks, max_points;
  int* counts;      // [n_chunks]: counts, then exclusive offsets
  float* points; double* points64; int* count;
};

// fp32 image: GridMap._map > threshold (grid_map.py:17).  int8 ROS image: -1 (unknown) -> 0, then fp32(v) / 100
// (grid_map.py:37-39); the quotient is formed in float64 and rounded, which equals the correctly rounded fp32 division.
template <class T>
__device__ __forceinline__ bool occupied(const GridArgs& a, int i) {
  if (i >= a.cells) return false;
  const T v = static_cast<const T*>(a.grid)[i];
  float f;
  if (sizeof(T) == 1) f = (float)((double)(v < 0 ? 0 : v) / 100.0);
  else f = (float)v;
  return f > a.threshold;
}

// grid_map.py:18-19 and Position2.apply (nfop/utils/position2.py:96-100) in float64, every operation rounded on its own
// like numpy's (hipcc would contract the plain expressions to fused multiply-adds)
__device__ __forceinline__ void cell_point(const GridArgs& a, int i, double* px, double* py) {
#pragma clang fp contract(off)
  const int row = i / a.cols, col = i - row * a.cols;
  const double x = (double)col * a.resolution + a.half, y = (double)row * a.resolution + a.half;
  const double xc = x * a.c, ys = y * a.s, xs = x * a.s, yc = y * a.c;
  const double dx = xc - ys, dy = xs + yc;
  *px = dx + a.ox;
  *py = dy + a.oy;
}

template <class T>
__global__ __launch_bounds__(OM_THREADS) void grid_count_kernel(const GridArgs a) {
  __shared__ int wave_n[OM_WAVES];
  const int base = blockIdx.x * GP_CHUNK + threadIdx.x;
  int n = 0;   // the same in every lane of a wave
#pragma unroll
  for (int t = 0; t < GP_TILES; ++t) n += __popcll(__ballot(occupied<T>(a, base + t * OM_THREADS)));
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
    for (int w = 0; w < OM_WAVES; ++w) all += wave_n[w];
    a.counts[blockIdx.x] = all;
  }
}

__global__ __launch_bounds__(OM_THREADS) void grid_scan_kernel(const GridArgs a) {
  __shared__ int wave_sums[OM_WAVES];
  int carry = 0;
  for (int base = 0; base < a.n_chunks; base += GP_SCAN_PASS) {
    const int i = base + threadIdx.x;
    const int v = i < a.n_chunks ? a.counts[i] : 0;
    int total;
    const int ex = block_exclusive_scan<OM_WAVES>(v, 0, Plus(), wave_sums, &total);
    if (i < a.n_chunks) a.counts[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *a.count = carry;
}

template <class T>
__global__ __launch_bounds__(OM_THREADS) void grid_emit_kernel(const GridArgs a) {
  __shared__ int wave_n[OM_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int run = a.counts[blockIdx.x];
  for (int t = 0; t < GP_TILES; ++t) {
    const int i = blockIdx.x * GP_CHUNK + t * OM_THREADS + threadIdx.x;
    const bool occ = occupied<T>(a, i);
    const unsigned long long m = __ballot(occ);
    __syncthreads();   // the previous tile's counts have been read
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < OM_WAVES; ++w) {
      before += w < wave ? wave_n[w] : 0;
      all += wave_n[w];
    }
    const int k = run + before + __popcll(m & ((1ull << lane) - 1ull));
    if (occ && k < a.max_points) {
      double x, y;
      cell_point(a, i, &x, &y);
      a.points[2 * k] = (float)x;
      a.points[2 * k + 1] = (float)y;
      if (a.points64) { a.points64[2 * k] = x; a.points64[2 * k + 1] = y; }
    }
    run += all;
  }
}

template <class T>
static int launch_grid_to_points(const GridArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(grid_count_kernel<T>, dim3(a.n_chunks), dim3(OM_THREADS), 0, st, a);
  hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(OM_THREADS), 0, st, a);
  if (a.max_points > 0) hipLaunchKernelGGL(grid_emit_kernel<T>, dim3(a.n_chunks), dim3(OM_THREADS), 0, st, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// ---- cell index: stable LSD radix sort of the points by their 16-bit cell id --------------------------------------
// Two 8-bit passes, each (1) digit histogram per segment of IX_SEGMENT consecutive points -- one wave per segment, its
// 256 counters in LDS --, (2) exclusive scan of the [digit][segment] table in that order by one workgroup, (3) scatter:
// each wave walks its segment again in the same order and stores every point at its digit's running offset.  Within a
// round of 64 points the lanes of one digit are found with 8 ballots, rank = popcount of the lower lanes, so equal keys
// keep their input order.  The key is recomputed from the point in every pass (it is a pure function of it), so only
// the points move.
constexpr int IX_ROUNDS = 8;
constexpr int IX_SEGMENT = 64 * IX_ROUNDS;            // 512 points per wave

struct IndexArgs {
  const float* in; float* out; int n, n_seg, shift;
  CellIndex index;   // its cell_start is what index_cell_start_kernel writes:
  int* cell_start;   // [cells_x * cells_y + 1]
  int* table;        // [256][n_seg]
};

// the sort key: the cell number the searching kernels will form for the same coordinates (CellIndex::cell)
__device__ __forceinline__ int cell_of(const IndexArgs& a, float x, float y) {
  int cx, cy;
  a.index.cell(x, y, &cx, &cy);
  return cy * a.index.cells_x + cx;
}

// lanes of the wave that hold a valid point with this lane's digit
__device__ __forceinline__ unsigned long long same_digit_lanes(int digit, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return valid ? peers : 0ull;
}

// SCATTER = false: table[digit][segment] <- count;  SCATTER = true: table holds the exclusive offsets, the points move
template <bool SCATTER>
__global__ __launch_bounds__(OM_THREADS) void index_pass_kernel(const IndexArgs a) {
  __shared__ int slot[OM_WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x * OM_WAVES + wave;
  const bool live = seg < a.n_seg;
  for (int d = lane; d < 256; d += 64) slot[wave][d] = (SCATTER && live) ? a.table[d * a.n_seg + seg] : 0;
  __syncthreads();
  for (int r = 0; r < IX_ROUNDS; ++r) {
    const long long i = (long long)seg * IX_SEGMENT + r * 64 + lane;
    const bool valid = live && i < a.n;
    float x = 0.f, y = 0.f;
    if (valid) { x = a.in[2 * i]; y = a.in[2 * i + 1]; }
    const int digit = (cell_of(a, x, y) >> a.shift) & 255;
    const unsigned long long peers = same_digit_lanes(digit, valid);
    const unsigned long long lower = peers & ((1ull << lane) - 1ull);
    int pos = 0;
    if (SCATTER && valid) pos = slot[wave][digit] + __popcll(lower);
    __syncthreads();   // every lane has read its offset before the digit's first lane advances it
    if (valid && lower == 0ull) slot[wave][digit] += __popcll(peers);
    __syncthreads();
    if (SCATTER && valid && pos < a.n) { a.out[2 * pos] = x; a.out[2 * pos + 1] = y; }
  }
  if (!SCATTER && live)
    for (int d = lane; d < 256; d += 64) a.table[d * a.n_seg + seg] = slot[wave][d];
}

// one thread per digit: its row of segment counts becomes the row of exclusive offsets (digit-major, segment-minor order)
__global__ __launch_bounds__(OM_THREADS) void index_scan_kernel(const IndexArgs a) {
  __shared__ int wave_sums[OM_WAVES];
  int* row = a.table + (long long)threadIdx.x * a.n_seg;
  int sum = 0;
  for (int s = 0; s < a.n_seg; ++s) sum += row[s];
  int run = block_exclusive_scan<OM_WAVES>(sum, 0, Plus(), wave_sums);
  for (int s = 0; s < a.n_seg; ++s) {
    const int t = row[s];
    row[s] = run;
    run += t;
  }
}

// cell_start[c] = first sorted point whose cell is >= c (np.searchsorted, side="left")
__global__ __launch_bounds__(OM_THREADS) void index_cell_start_kernel(const IndexArgs a) {
  const int c = blockIdx.x * OM_THREADS + threadIdx.x;
  if (c > a.index.cells_x * a.index.cells_y) return;
  int lo = 0, hi = a.n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cell_of(a, a.in[2 * (long long)mid], a.in[2 * (long long)mid + 1]) < c) lo = mid + 1;
    else hi = mid;
  }
  a.cell_start[c] = lo;
}

static StreamScratch<> g_grid_counts;

static size_t index_table_bytes(int64_t n) { return (size_t)256 * (size_t)((n + IX_SEGMENT - 1) / IX_SEGMENT) * sizeof(int); }
static size_t index_points_bytes(int64_t n) { return ((size_t)n * 2 * sizeof(float) + 255) & ~(size_t)255; }

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_grid_to_points(const void* grid_dev, int32_t is_int8, int32_t rows, int32_t cols, float threshold,
                                    double resolution, double origin_x, double origin_y, double origin_cos,
                                    double origin_sin, int32_t max_points, float* points_dev, double* points64_dev,
                                    int32_t* count_dev, void* stream) {
  NFOPP_REQUIRE(rows > 0 && cols > 0, "need a grid of at least one cell");
  NFOPP_REQUIRE((long long)rows * cols <= GP_MAX_CELLS, "grids of more than 2^24 cells are not supported");
  NFOPP_REQUIRE(max_points >= 0, "negative max_points");
  NFOPP_REQUIRE(grid_dev && count_dev && (max_points == 0 || points_dev), "null device pointer");
  GridArgs a = {};
  a.grid = grid_dev; a.cells = rows * cols; a.cols = cols; a.threshold = threshold;
  a.resolution = resolution; a.half = resolution / 2.0; a.ox = origin_x; a.oy = origin_y; a.c = origin_cos; a.s = origin_sin;
  a.n_chunks = (a.cells + GP_CHUNK - 1) / GP_CHUNK; a.max_points = max_points;
  a.points = points_dev; a.points64 = points64_dev; a.count = count_dev;
  void* counts = nullptr;
  const int rc = g_grid_counts.acquire((size_t)a.n_chunks * sizeof(int), (hipStream_t)stream, &counts);
  if (rc != NFOPP_OK) return rc;
  a.counts = static_cast<int*>(counts);
  return is_int8 ? launch_grid_to_points<signed char>(a, (hipStream_t)stream)
                 : launch_grid_to_points<float>(a, (hipStream_t)stream);
}

extern "C" size_t nfopp_cell_index_workspace_bytes(int32_t n_obstacles) {
  if (n_obstacles <= 0) return 0;
  return index_points_bytes(n_obstacles) + index_table_bytes(n_obstacles);
}

extern "C" int nfopp_build_cell_index(const float* obstacles_dev, int32_t n_obstacles, float cell_x0, float cell_y0,
                                      float cell_size, int32_t cells_x, int32_t cells_y, float* obstacles_sorted_dev,
                                      int32_t* cell_start_dev, void* workspace_dev, size_t workspace_bytes,
                                      void* stream) {
  NFOPP_REQUIRE(n_obstacles >= 0, "negative obstacle count");
  IndexArgs a = {};
  const int rc = fill_cell_index(&a.index, cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size);
  if (rc) return rc;
  NFOPP_REQUIRE((long long)cells_x * cells_y <= MAX_INDEX_CELLS, "the index holds between 1 and 65536 cells");
  hipStream_t st = (hipStream_t)stream;
  const int cells = cells_x * cells_y;
  if (n_obstacles == 0) {
    NFOPP_HIP(hipMemsetAsync(cell_start_dev, 0, (size_t)(cells + 1) * sizeof(int32_t), st));
    return NFOPP_OK;
  }
  NFOPP_REQUIRE(obstacles_dev && obstacles_sorted_dev && workspace_dev, "null device pointer");
  NFOPP_REQUIRE(workspace_bytes >= nfopp_cell_index_workspace_bytes(n_obstacles),
                "workspace smaller than nfopp_cell_index_workspace_bytes");
  a.n = n_obstacles; a.n_seg = (n_obstacles + IX_SEGMENT - 1) / IX_SEGMENT;
  float* tmp = static_cast<float*>(workspace_dev);
  a.table = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + index_points_bytes(n_obstacles));
  a.cell_start = cell_start_dev;
  const unsigned grid = (unsigned)((a.n_seg + OM_WAVES - 1) / OM_WAVES);
  for (int pass = 0; pass < 2; ++pass) {   // low byte: obstacles -> workspace, high byte: workspace -> sorted
    a.in = pass == 0 ? obstacles_dev : tmp;
    a.out = pass == 0 ? tmp : obstacles_sorted_dev;
    a.shift = 8 * pass;
    hipLaunchKernelGGL(index_pass_kernel<false>, dim3(grid), dim3(OM_THREADS), 0, st, a);
    hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(OM_THREADS), 0, st, a);
    hipLaunchKernelGGL(index_pass_kernel<true>, dim3(grid), dim3(OM_THREADS), 0, st, a);
  }
  a.in = obstacles_sorted_dev;
  hipLaunchKernelGGL(index_cell_start_kernel, dim3((unsigned)(cells + 1 + OM_THREADS - 1) / OM_THREADS), dim3(OM_THREADS), 0,
                     st, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
