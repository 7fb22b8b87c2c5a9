// Batched shortest-path seeding on an occupancy grid: B (start, goal) problems on one shared grid -> B initial
// trajectories, in three stages (distance fields, path trace, spline seeding).
//
// Replaces AstarTrajectoryInitializer.initialize_trajectory / calculate_astar_path
// (nfop/astar/astar_trajectory_initializer.py:15-48), the search of nfop/astar/jps.py with jps=False (8-connected,
// cost 1 / sqrt 2, no corner rule: jps.py:99-125, cells outside the matrix are walls) and reparametrize_path
// (nfop/utils/math.py:57-65).  The reference runs one heap search per problem; its heuristic is consistent, so it
// returns A minimum-cost path, and which one depends on its heap order.  Here the search is a cost-to-goal field per
// distinct goal cell, shared by every problem with that goal, and a descent through it per problem.
//
// A cost is the integer pair (a, b) = (straight moves, diagonal moves).  sqrt 2 is irrational, so two paths of equal
// cost have the same pair, and with exact ordering of pairs the field is the unique fixed point of
//   d(c) = min over free neighbours n of d(n) + move(n, c),   d(goal) = (0, 0):
// any relaxation schedule reaches the same bits.  Pairs are ordered by a + b * sqrt 2 in float64: for counts below 2^21
// two different pairs differ by more than 1 / (2^21 * 2.42) = 2e-7 while the rounding of the key (and of the few
// additions made on it inside one sweep) stays below 3e-9, so the order of DIFFERENT pairs is exact; whether a cell
// changed is decided on the integer pair itself.
#include "common.h"
#include "grid_frame.h"
#include "lattice_field.h"
#include "pair_cost.h"
#include "spline2.h"
#include "traj_init.h"

namespace nfopp {

constexpr int GS_THREADS = 512;
constexpr int GS_RUN = 7;             // cells a thread relaxes at a time (odd: conflict-free ds_read_b32 across lanes)
constexpr int GS_LDS_WORDS = 36864;   // packed field in LDS up to 144 KiB

template <class T>
__device__ __forceinline__ void take_min(double& best_k, T& best_v, double k, T v, double cost, T inc) {
  const double ck = k + cost;   // inf stays inf
  if (ck < best_k) { best_k = ck; best_v = v + inc; }
}

struct FieldArgs {
  const unsigned char* occ;   // [rows, cols]
  const int* goals;           // [G, 2] (row, col)
  int rows, cols, cols_p, stride;
  long long padded;           // cells of one padded field
  int* out;                   // [G, rows, cols, 2]
  void* work;                 // wide path: G padded fields of uint64
};

// One workgroup per goal.  F is the padded field: (rows + 2) x stride cells, a wall border all round and the columns
// padded to a multiple of GS_RUN, so no access below needs a bounds test.  A thread takes runs of GS_RUN cells of one
// row: it reads the run with one halo cell either side and the rows above and below it (3 reads per cell instead of
// 8), folds the six outer neighbours of every cell into one candidate, relaxes the run left-to-right and right-to-left
// in registers (a cost crosses the run in one sweep) and stores the cells that changed.  Sweeps are in place and
// unsynchronised inside: every value ever stored is the cost of a real path and values only fall, so a sweep in which no
// cell changed (tested over the workgroup) is the fixed point.  After k sweeps the k nearest cells are final, so at most
// rows * cols sweeps are made.
template <class T>
__device__ __forceinline__ void field_body(const FieldArgs& a, T* F, int g) {
  using P = Packed<T>;
  const int rows = a.rows, cols = a.cols, stride = a.stride;
  const int gr = a.goals[2 * g], gc = a.goals[2 * g + 1];
  const bool goal_ok = gr >= 0 && gr < rows && gc >= 0 && gc < cols;
  // the padded field of lattice_field.h, one layer; the goal cell is forced free (astar_trajectory_initializer.py:40)
  lattice_fill_layer<T, GS_THREADS>(F, a.occ, rows, cols, stride, a.padded, gr, gc, true);
  if (sizeof(T) == 8) __threadfence();
  __syncthreads();
  const int runs_per_row = a.cols_p / GS_RUN;
  const long long n_runs = (long long)rows * runs_per_row;
  const long long max_sweeps = (long long)rows * cols + 1;
  for (long long sweep = 0; goal_ok && sweep < max_sweeps; ++sweep) {
    int changed = 0;
    for (long long q = threadIdx.x; q < n_runs; q += GS_THREADS) {
      const int r = (int)(q / runs_per_row), c0 = (int)(q % runs_per_row) * GS_RUN;
      T* mid_p = F + (long long)(r + 1) * stride + c0;   // column c0 - 1 of row r
      const T* up_p = mid_p - stride;
      const T* dn_p = mid_p + stride;
      T mid[GS_RUN + 2], ext_v[GS_RUN + 2];
      double mid_k[GS_RUN + 2], ext_k[GS_RUN + 2];
      bool any_free = false;
#pragma unroll
      for (int j = 0; j < GS_RUN + 2; ++j) {
        mid[j] = mid_p[j];
        mid_k[j] = pair_key(mid[j]);
        if (j >= 1 && j <= GS_RUN) any_free |= mid[j] != P::WALL;
      }
      if (!any_free) continue;
      {
        T up[GS_RUN + 2], dn[GS_RUN + 2];
        double up_k[GS_RUN + 2], dn_k[GS_RUN + 2];
#pragma unroll
        for (int j = 0; j < GS_RUN + 2; ++j) {
          up[j] = up_p[j]; dn[j] = dn_p[j];
          up_k[j] = pair_key(up[j]); dn_k[j] = pair_key(dn[j]);
        }
#pragma unroll
        for (int j = 1; j <= GS_RUN; ++j) {
          double k = INFINITY;
          T v = P::UNREACHED;
          take_min(k, v, up_k[j], up[j], 1.0, P::STRAIGHT);
          take_min(k, v, dn_k[j], dn[j], 1.0, P::STRAIGHT);
          take_min(k, v, up_k[j - 1], up[j - 1], GS_SQRT2, P::DIAGONAL);
          take_min(k, v, up_k[j + 1], up[j + 1], GS_SQRT2, P::DIAGONAL);
          take_min(k, v, dn_k[j - 1], dn[j - 1], GS_SQRT2, P::DIAGONAL);
          take_min(k, v, dn_k[j + 1], dn[j + 1], GS_SQRT2, P::DIAGONAL);
          ext_k[j] = k; ext_v[j] = v;
        }
      }
      T was[GS_RUN + 2];
#pragma unroll
      for (int j = 1; j <= GS_RUN; ++j) was[j] = mid[j];
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int jj = 1; jj <= GS_RUN; ++jj) {
          const int j = pass == 0 ? jj : GS_RUN + 1 - jj;
          if (mid[j] == P::WALL) continue;
          double k = mid_k[j];
          T v = mid[j];
          if (pass == 0 && ext_k[j] < k) { k = ext_k[j]; v = ext_v[j]; }
          take_min(k, v, mid_k[j - 1], mid[j - 1], 1.0, P::STRAIGHT);
          take_min(k, v, mid_k[j + 1], mid[j + 1], 1.0, P::STRAIGHT);
          mid[j] = v; mid_k[j] = k;
        }
      }
#pragma unroll
      for (int j = 1; j <= GS_RUN; ++j)
        if (mid[j] != was[j]) { mid_p[j] = mid[j]; changed = 1; }
    }
    if (sizeof(T) == 8) __threadfence();   // wide path: the field lives in global memory, the next sweep must not read stale lines
    if (!__syncthreads_or(changed)) break;
  }
  lattice_store_layer<T, GS_THREADS>(F, 0, reinterpret_cast<int2*>(a.out + (long long)g * rows * cols * 2), 0, (long long)rows * cols, cols,
                                     stride);
}

__global__ __launch_bounds__(GS_THREADS) void field_lds_kernel(const FieldArgs a) {
  extern __shared__ uint32_t gs_lds[];
  field_body<uint32_t>(a, gs_lds, blockIdx.x);
}

__global__ __launch_bounds__(GS_THREADS) void field_wide_kernel(const FieldArgs a) {
  field_body<uint64_t>(a, reinterpret_cast<uint64_t*>(a.work) + (long long)blockIdx.x * a.padded, blockIdx.x);
}

// ---- stage 2: descent through the field, one problem per thread ------------------------------------------------------
// Neighbour order (row, col), the order of jps.py:99-113: N, W, S, E, NW, NE, SW, SE.  The first neighbour in this order
// with d(n) + move == d(current), as integer equality on the pair, is taken.
__constant__ int GS_DR[8] = {-1, 0, 1, 0, -1, -1, 1, 1};
__constant__ int GS_DC[8] = {0, -1, 0, 1, -1, 1, -1, 1};

struct TraceArgs {
  const int* fields;        // [G, rows, cols, 2]
  const int* start_cells;   // [B, 2]
  const int* goal_cells;    // [B, 2]
  const int* field_index;   // [B]
  int rows, cols, max_len;
  long long batch, n_fields;
  int* cells;               // [B, max_len, 2]
  int* count; int* status; int* cost;
};

__global__ __launch_bounds__(256) void trace_kernel(const TraceArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.batch) return;
  const int rows = a.rows, cols = a.cols;
  int r = a.start_cells[2 * p], c = a.start_cells[2 * p + 1];
  const int gr = a.goal_cells[2 * p], gc = a.goal_cells[2 * p + 1];
  const long long fi = a.field_index[p];
  int status = 0, count = 0, ca = -1, cb = -1;
  if (r < 0 || r >= rows || c < 0 || c >= cols || gr < 0 || gr >= rows || gc < 0 || gc >= cols || fi < 0 || fi >= a.n_fields) {
    status = 2;
  } else {
    const int2* f = reinterpret_cast<const int2*>(a.fields) + fi * rows * cols;
    int2* cells = a.max_len > 0 ? reinterpret_cast<int2*>(a.cells) + p * a.max_len : nullptr;
    int2 d = f[(long long)r * cols + c];
    int len = 0;
    if (d.x < 0) {
      // the start cell is not tested for occupancy (astar_trajectory_initializer.py:41-42 starts the search there):
      // from a wall cell the first move goes to the best free neighbour
      double best = INFINITY;
      int bi = -1;
      int2 bd = d;
      for (int i = 0; i < 8; ++i) {
        const int nr = r + GS_DR[i], nc = c + GS_DC[i];
        if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
        const int2 dn = f[(long long)nr * cols + nc];
        if (dn.x < 0) continue;
        const int na = dn.x + (i < 4), nb = dn.y + (i >= 4);
        const double k = pair_key(na, nb);
        if (k < best && !(bi >= 0 && na == bd.x && nb == bd.y)) { best = k; bi = i; bd.x = na; bd.y = nb; }
      }
      if (bi < 0) status = 1;
      else {
        if (cells && len < a.max_len) cells[len] = make_int2(r, c);
        ++len;
        ca = bd.x; cb = bd.y;
        r += GS_DR[bi]; c += GS_DC[bi];
        d = f[(long long)r * cols + c];
      }
    } else {
      ca = d.x; cb = d.y;
    }
    if (status == 0) {
      count = len + d.x + d.y + 1;
      if (cells) {
        int left = d.x + d.y;   // every move lowers a + b by one: the walk ends
        for (;;) {
          if (len < a.max_len) cells[len] = make_int2(r, c);
          ++len;
          if (left == 0) break;
          int pick = -1;
          int2 dn = d;
          for (int i = 0; i < 8 && pick < 0; ++i) {
            const int nr = r + GS_DR[i], nc = c + GS_DC[i];
            if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
            dn = f[(long long)nr * cols + nc];
            if (dn.x >= 0 && dn.x + (i < 4) == d.x && dn.y + (i >= 4) == d.y) pick = i;
          }
          if (pick < 0) break;   // cannot happen on a fixed-point field; count then exceeds what was written
          r += GS_DR[pick]; c += GS_DC[pick];
          d = dn;
          --left;
        }
      }
    }
  }
  a.count[p] = count;
  a.status[p] = status;
  if (a.cost) { a.cost[2 * p] = ca; a.cost[2 * p + 1] = cb; }
}

// ---- stage 3: polyline -> spline -> waypoints ------------------------------------------------------------------------
constexpr int SD_THREADS = 256;

struct SeedArgs {
  const int* cells; const int* count; const int* status;
  const float* points;      // [B, max_len, 2] fp32 xy: the interior of the polyline as given (cells is then null), else null
  const int* headings = nullptr;   // [B, max_len] lattice headings of the cells: theta is then the body heading of the path
  int max_len, n, directed;
  const float* start; const float* goal;
  double ox, oy, res;
  float* traj;
  double* work;             // global workspace, or null: dynamic LDS
  long long work_stride;    // doubles per problem
};

// numpy's arithmetic on the fp32 polyline (math.py:58-61): fp32 segment lengths + 1e-6 and their fp32 running sum, the
// parameter and everything after it in float64; no fused multiply-adds
#pragma clang fp contract(off)

template <int D>
__device__ __forceinline__ void seed_body(const SeedArgs& a, double* W, long long b) {
  const int N = a.n;
  float s[D], g[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { s[d] = a.start[b * D + d]; g[d] = a.goal[b * D + d]; }
  float* out = a.traj + b * (long long)N * D;
  const int cnt = a.count[b];
  if (a.status[b] != 0 || cnt < 1 || cnt > a.max_len) {
    // unreachable goal, endpoints off the grid: exactly the stock initialiser's trajectory
    straight_line_fill<D>(s, g, N, a.directed, out, threadIdx.x, SD_THREADS);
    return;
  }
  const int m = cnt + 2;
  const SplineArea sp = spline_carve<2>(W, a.max_len + 2);
  double* C = sp.C;
  const double *T = sp.T, *PAR = sp.PAR;
  float* P = reinterpret_cast<float*>(sp.end);   // 2m polyline (fp32, as the reference builds it)
  const int2* cells = reinterpret_cast<const int2*>(a.cells) + b * (long long)a.max_len;
  const float* points = a.points ? a.points + b * (long long)a.max_len * 2 : nullptr;
  // polyline = [start, cell centres, goal] (astar_trajectory_initializer.py:19-20, 45-47: centres in float64, stored fp32)
  for (int k = threadIdx.x; k < m; k += SD_THREADS) {
    float x, y;
    if (k == 0) { x = s[0]; y = s[1]; }
    else if (k == m - 1) { x = g[0]; y = g[1]; }
    else if (points) { x = points[2 * (k - 1)]; y = points[2 * (k - 1) + 1]; }
    else {
      const int2 rc = cells[k - 1];
      x = grid_cell_centre((double)rc.y, a.res, a.ox);
      y = grid_cell_centre((double)rc.x, a.res, a.oy);
    }
    P[2 * k] = x; P[2 * k + 1] = y;
    C[2 * k] = (double)x; C[2 * k + 1] = (double)y;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    // whether the sites are distinct is not looked at: two equal ones give NaN waypoints with status 0 (open)
    chord_parameter<2>(P, m, sp.PAR, nullptr);
    spline_fit<2>(sp, m);
  }
  __threadfence_block();
  __syncthreads();
  // np.linspace(0, 1, N + 2)[1:-1]: q * step in float64
  const double step = 1.0 / (double)(N + 1);
  for (int i = threadIdx.x; i < N; i += SD_THREADS) {
    double p[2];
    spline_at<2>(T, C, m, (double)(i + 1) * step, p);
    out[i * D + 0] = (float)p[0];
    out[i * D + 1] = (float)p[1];
  }
  if (D == 3 && a.headings) {
    // The body heading of a lattice path (nfopp_lattice_seed_trajectories), unwound and interpolated over the spline's own
    // parameter; float64, every operation rounded on its own, no atan2 / sin / cos.  Knots A[0 .. m - 1]: the start angle,
    // the cells' headings as a1 + u_k * (pi / 4) with u the running sum of the signed heading steps, the goal angle; a1 and
    // the goal knot are the nearest turn to the knot before them, wrap(x) = x - 2 pi * rint(x / 2 pi).
    double* A = sp.DD;   // the pivots are done with
    if (threadIdx.x == 0) {
      const int* heads = a.headings + b * (long long)a.max_len;
      const double quarter = NFOPP_PI_D / 4.0, two_pi = 2.0 * NFOPP_PI_D;
      const double ths = (double)s[2];
      double x = (double)heads[0] * quarter - ths;
      const double a1 = ths + (x - two_pi * rint(x / two_pi));
      int u = 0;
      A[0] = ths;
      A[1] = a1 + (double)u * quarter;
      for (int k = 1; k < cnt; ++k) {
        u += ((heads[k] - heads[k - 1] + 4) & 7) - 4;   // -1, 0 or +1 between the states of a lattice path
        A[k + 1] = a1 + (double)u * quarter;
      }
      x = (double)g[2] - A[cnt];
      A[m - 1] = A[cnt] + (x - two_pi * rint(x / two_pi));
    }
    __threadfence_block();
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += SD_THREADS) {
      const double q = (double)(i + 1) * step;   // the parameter the xy spline is evaluated at
      int lo = 0, hi = m - 2;                    // largest k in [0, m - 2] with PAR[k] <= q: PAR[k + 1] > q, as q < 1
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (PAR[mid] <= q) lo = mid; else hi = mid - 1;
      }
      const double w = (q - PAR[lo]) / (PAR[lo + 1] - PAR[lo]);
      out[i * D + 2] = (float)(A[lo] + (A[lo + 1] - A[lo]) * w);
    }
  } else if (D == 3) {
    __threadfence_block();
    __syncthreads();
    // initialize_angle / initialize_angle_with_trajectory_direction (trajectory_initializer.py:23-45) on the seeded xy
    const int steps = N + 2;
    const float goal_angle = wrap_angle(g[2] - s[2]) + s[2];
    for (int i = threadIdx.x; i < N; i += SD_THREADS) {
      float th = linspace_at(s[2], goal_angle, steps, i + 1);
      if (a.directed) {
        const float x0 = i == 0 ? s[0] : out[(i - 1) * D], y0 = i == 0 ? s[1] : out[(i - 1) * D + 1];
        const float x1 = i == N - 1 ? g[0] : out[(i + 1) * D], y1 = i == N - 1 ? g[1] : out[(i + 1) * D + 1];
        const float heading = atan2f(y1 - y0, x1 - x0);
        const int h = N / 2;
        const float w = i < h ? linspace_at(0.f, 1.f, h, i) : linspace_at(1.f, 0.f, (N + 1) / 2, i - h);
        th = add_mul_unfused(th, wrap_angle(heading - th), w);
      }
      out[i * D + 2] = th;
    }
  }
}

template <int D>
__global__ __launch_bounds__(SD_THREADS) void seed_kernel(const SeedArgs a) {
  extern __shared__ double sd_lds[];
  const long long b = blockIdx.x;
  if (a.work) seed_body<D>(a, a.work + b * a.work_stride, b);
  else seed_body<D>(a, sd_lds, b);
}

// doubles one problem needs: the spline's area for M = max_len + 2 sites of xy, and behind it the fp32 polyline, 2M floats
static long long seed_doubles(int max_len) { return spline_doubles(max_len + 2, 2) + (max_len + 2); }
constexpr long long SD_LDS_BYTES = 64 * 1024;

static bool field_fits_lds(int rows, int cols, int* cols_p, int* stride, long long* padded) {
  *cols_p = (cols + GS_RUN - 1) / GS_RUN * GS_RUN;
  *stride = *cols_p + 2;
  *padded = (long long)(rows + 2) * *stride;
  return (long long)rows * cols <= 65535 && *padded <= GS_LDS_WORDS;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_grid_fields_workspace_bytes(int32_t rows, int32_t cols, int64_t n_goals) {
  if (rows < 1 || cols < 1 || n_goals < 1) return 0;
  int cols_p, stride;
  long long padded;
  if (field_fits_lds(rows, cols, &cols_p, &stride, &padded)) return 0;
  return (size_t)padded * 8 * (size_t)n_goals;
}

extern "C" int nfopp_grid_distance_fields(const uint8_t* occupancy_dev, int32_t rows, int32_t cols,
                                          const int32_t* goal_cells_dev, int64_t n_goals, int32_t* fields_dev,
                                          void* workspace_dev, size_t workspace_bytes, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768, "grid must be 1..32768 cells a side");
  // counts are int32 and the float64 order of pairs is exact below 2^21 moves: no path of such a grid is longer
  NFOPP_REQUIRE((long long)rows * cols <= (1LL << 21), "grid has more than 2^21 cells: path counts could leave the exactly ordered range");
  NFOPP_REQUIRE(n_goals >= 0 && n_goals <= 0x7fffffffLL, "bad goal count");
  if (n_goals == 0) return NFOPP_OK;
  NFOPP_REQUIRE(occupancy_dev && goal_cells_dev && fields_dev, "null device pointer");
  FieldArgs a;
  a.occ = occupancy_dev; a.goals = goal_cells_dev; a.rows = rows; a.cols = cols; a.out = fields_dev; a.work = nullptr;
  if (field_fits_lds(rows, cols, &a.cols_p, &a.stride, &a.padded)) {
    static bool attr_set[MAX_DEVICES] = {};
    const size_t lds = (size_t)a.padded * 4;
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(field_lds_kernel), (size_t)GS_LDS_WORDS * 4, attr_set);
    if (rc != NFOPP_OK) return rc;
    hipLaunchKernelGGL(field_lds_kernel, dim3((unsigned)n_goals), dim3(GS_THREADS), lds, (hipStream_t)stream, a);
  } else {
    const size_t need = (size_t)a.padded * 8 * (size_t)n_goals;
    NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small: nfopp_grid_fields_workspace_bytes gives %zu", need);
    a.work = workspace_dev;
    hipLaunchKernelGGL(field_wide_kernel, dim3((unsigned)n_goals), dim3(GS_THREADS), 0, (hipStream_t)stream, a);
  }
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_grid_trace_paths(const int32_t* fields_dev, int64_t n_fields, int32_t rows, int32_t cols,
                                      const int32_t* start_cells_dev, const int32_t* goal_cells_dev,
                                      const int32_t* field_index_dev, int64_t batch, int32_t max_len, int32_t* cells_dev,
                                      int32_t* count_dev, int32_t* status_dev, int32_t* cost_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && n_fields >= 0 && max_len >= 0, "bad sizes");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL, "bad batch");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(start_cells_dev && goal_cells_dev && field_index_dev && count_dev && status_dev, "null device pointer");
  NFOPP_REQUIRE((fields_dev || n_fields == 0) && (cells_dev || max_len == 0), "null device pointer");
  TraceArgs a;
  a.fields = fields_dev; a.start_cells = start_cells_dev; a.goal_cells = goal_cells_dev; a.field_index = field_index_dev;
  a.rows = rows; a.cols = cols; a.max_len = max_len; a.batch = batch; a.n_fields = n_fields;
  a.cells = cells_dev; a.count = count_dev; a.status = status_dev; a.cost = cost_dev;
  hipLaunchKernelGGL(trace_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" size_t nfopp_grid_seed_workspace_bytes(int64_t batch, int32_t max_len) {
  if (batch < 1 || max_len < 1) return 0;
  const long long bytes = seed_doubles(max_len) * 8;
  return bytes <= SD_LDS_BYTES ? 0 : (size_t)bytes * (size_t)batch;
}

// the launch both seeding entries share: `a` holds the source of the polyline's interior (cells or points) and its geometry
static int seed_launch(SeedArgs a, const int32_t* count_dev, const int32_t* status_dev, int64_t batch, int32_t max_len,
                       const float* start_dev, const float* goal_dev, int32_t n_waypoints, int32_t dim,
                       int32_t angles_with_direction, float* traj_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && n_waypoints >= 1 && max_len >= 0, "bad sizes");
  NFOPP_REQUIRE(max_len <= (1 << 21) + 1, "path buffer longer than any path of a supported grid");
  NFOPP_REQUIRE(!(angles_with_direction && dim != 3), "heading initialisation needs SE(2) trajectories (dim 3)");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(count_dev && status_dev && start_dev && goal_dev && traj_dev && (a.cells || a.points || max_len == 0),
                "null device pointer");
  a.count = count_dev; a.status = status_dev; a.max_len = max_len; a.n = n_waypoints;
  a.directed = angles_with_direction ? 1 : 0; a.start = start_dev; a.goal = goal_dev; a.traj = traj_dev;
  a.work = nullptr; a.work_stride = seed_doubles(max_len);
  size_t lds = (size_t)a.work_stride * 8;
  if ((long long)lds > SD_LDS_BYTES) {
    const size_t need = lds * (size_t)batch;
    NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small: nfopp_grid_seed_workspace_bytes gives %zu", need);
    NFOPP_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace must be 8-byte aligned");
    a.work = reinterpret_cast<double*>(workspace_dev);
    lds = 0;
  }
  if (dim == 3) hipLaunchKernelGGL(seed_kernel<3>, dim3((unsigned)batch), dim3(SD_THREADS), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(seed_kernel<2>, dim3((unsigned)batch), dim3(SD_THREADS), lds, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_grid_seed_trajectories(const int32_t* cells_dev, const int32_t* count_dev, const int32_t* status_dev,
                                            int64_t batch, int32_t max_len, const float* start_dev, const float* goal_dev,
                                            int32_t n_waypoints, int32_t dim, int32_t angles_with_direction,
                                            double origin_x, double origin_y, double resolution, float* traj_dev,
                                            void* workspace_dev, size_t workspace_bytes, void* stream) {
  NFOPP_REQUIRE(resolution > 0.0, "bad resolution");
  SeedArgs a;
  a.cells = cells_dev; a.points = nullptr; a.ox = origin_x; a.oy = origin_y; a.res = resolution;
  return seed_launch(a, count_dev, status_dev, batch, max_len, start_dev, goal_dev, n_waypoints, dim, angles_with_direction,
                     traj_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int nfopp_grid_seed_polylines(const float* points_dev, const int32_t* count_dev, const int32_t* status_dev,
                                         int64_t batch, int32_t max_len, const float* start_dev, const float* goal_dev,
                                         int32_t n_waypoints, int32_t dim, int32_t angles_with_direction, float* traj_dev,
                                         void* workspace_dev, size_t workspace_bytes, void* stream) {
  SeedArgs a;
  a.cells = nullptr; a.points = points_dev; a.ox = a.oy = 0.0; a.res = 1.0;   // the geometry is in the points already
  return seed_launch(a, count_dev, status_dev, batch, max_len, start_dev, goal_dev, n_waypoints, dim, angles_with_direction,
                     traj_dev, workspace_dev, workspace_bytes, stream);
}

// The seeding stage for lattice paths (lattice_search.hip, lattice_gears.hip): xy as nfopp_grid_seed_trajectories writes it for
// the same cells, theta from the headings of the lattice states, so a reverse run keeps the body heading it is driven at.
extern "C" size_t nfopp_lattice_seed_workspace_bytes(int64_t batch, int32_t max_len) {
  return nfopp_grid_seed_workspace_bytes(batch, max_len);
}

extern "C" int nfopp_lattice_seed_trajectories(const int32_t* cells_dev, const int32_t* headings_dev, const int32_t* count_dev,
                                               const int32_t* status_dev, int64_t batch, int32_t max_len, const float* start_dev,
                                               const float* goal_dev, int32_t n_waypoints, double origin_x, double origin_y,
                                               double resolution, float* traj_dev, void* workspace_dev, size_t workspace_bytes,
                                               void* stream) {
  NFOPP_REQUIRE(resolution > 0.0, "bad resolution");
  NFOPP_REQUIRE(batch <= 0 || max_len <= 0 || (cells_dev && headings_dev), "null device pointer");
  SeedArgs a;
  a.cells = cells_dev; a.points = nullptr; a.headings = headings_dev; a.ox = origin_x; a.oy = origin_y; a.res = resolution;
  return seed_launch(a, count_dev, status_dev, batch, max_len, start_dev, goal_dev, n_waypoints, 3, 0, traj_dev, workspace_dev,
                     workspace_bytes, stream);
}
