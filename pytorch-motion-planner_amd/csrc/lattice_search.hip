// Heading-aware lattice search for car-like trajectory seeds: cost-to-goal fields over (cell, heading) states and a
// descent through them per problem.  The traced cells go through nfopp_grid_seed_trajectories unchanged.  The rule is this
// library's own (the reference has no such search); it is stated here, in include/nfopp_hip.h and in tests/lattice_ref.py.
//
// STATE.  (cell (row, col), heading h in 0 .. 7); heading h stands for the angle h * pi / 4.
// DIRECTIONS.  dir(h) as (d row, d col), row = y and col = x as in the occupancy grid:
//   h      0       1       2       3       4        5        6       7
//   dir  (0,+1)  (+1,+1)  (+1,0)  (+1,-1)  (0,-1)  (-1,-1)  (-1,0)  (-1,+1)
// OCCUPANCY.  layers uint8 [L, rows, cols], L = 1 or 8, non-zero = blocked; state (c, h) reads layer h mod L; cells
//   outside the image are blocked; no corner rule between states.
// MOVES.  Forward only: from (c, h) to (c + dir(h'), h') with h' in {h, h + 1, h - 1} mod 8 -- the move is along the heading
//   the robot has AFTER it, which differs from the one before by at most one step.  The target state must be free.
// COST.  An integer pair (a, b) ordered exactly as a + b * sqrt 2 (pair_cost.h).  A move to an even h' adds (1, 0), to an
//   odd h' (0, 1); a move with h' != h adds a further (turn_cost, 0), turn_cost an integer 0 .. 255.  Equal cost means
//   equal pair, so the field is the unique fixed point of the relaxation and is compared with ==.
// GOAL.  (goal cell, goal heading); with goal heading -1 the goal cell at every heading.  Goal states have cost (0, 0) and
//   are forced free.
// FIELD.  d_g(c, h) = the minimum cost from (c, h) to g.  The sentinel (-1, -1) marks blocked states, states that cannot
//   reach g, and every state of a goal whose cell is outside the grid or whose heading is outside -1 .. 7.
// TRACE.  Problem p starts in (start cell, start heading); the start state is NOT tested for occupancy.  At a state with a
//   cost the next state is the first successor, tried in the order h' = h, h + 1, h - 1, whose cost plus the move equals
//   the current cost exactly; the trace ends at the first state with cost (0, 0).  At a start state whose own value is the
//   sentinel (a blocked start) the first step goes to the successor with the smallest d + move, ties broken by the same
//   order; the path's cost is that sum; if no successor has a cost the status is 1.
// STATUS.  0 ok; 1 unreachable; 2 the start or goal cell is outside the grid, or the start heading is outside 0 .. 7.
// REFUSED before launch, nothing is clamped: turn_cost outside 0 .. 255, L not 1 or 8, 8 * rows * cols * (1 + turn_cost) >=
//   2^21 (the bound under which the float64 key orders pairs exactly), a short workspace, null required pointers.
#include "common.h"
#include "pair_cost.h"

namespace nfopp {

constexpr int LS_THREADS = 512;
constexpr int LS_HEADINGS = 8;
constexpr int LS_BATCH = 4;             // cells of a line a thread has in flight: their 3 reads each are issued before any is used
constexpr int LS_LDS_WORDS = 36864;     // packed 8-layer field in LDS up to 144 KiB
constexpr long long LS_MAX_COUNT = 1LL << 21;

__constant__ int LS_DR[LS_HEADINGS] = {0, 1, 1, 1, 0, -1, -1, -1};
__constant__ int LS_DC[LS_HEADINGS] = {1, 1, 0, -1, -1, -1, 0, 1};

struct LatticeFieldArgs {
  const unsigned char* occ;   // [L, rows, cols]
  const int* goals;           // [G, 3] (row, col, heading or -1)
  int layers, rows, cols, stride, turn_cost;
  long long padded;           // cells of one padded layer
  int* out;                   // [G, 8, rows, cols, 2]
  void* work;                 // wide path: G padded 8-layer fields of uint64
};

// One workgroup per goal state.  F holds 8 padded layers of (rows + 2) x stride cells with a blocked border all round, so
// the successors of a cell of the image are read without a bounds test.  A thread takes a LINE of one layer: the cells of
// layer h along dir(h) -- a row for h = 0, 4, a column for h = 2, 6, a diagonal for odd h -- and walks it against the
// heading from its far end, the straight successor's value carried in a register: a straight run of any length settles in
// ONE sweep, so the sweeps a field needs follow the turns of its paths, not their lengths.  Per cell the walk reads the
// state itself and the two turn successors (layers h + 1 and h - 1), LS_BATCH cells ahead of the arithmetic.  Lanes hold
// neighbouring lines: their reads are consecutive cells (columns, diagonals from the far row) or `stride` apart (rows,
// diagonals from the far column), and stride is odd, so a half-wave of ds_read_b32 never meets twice on one of the 32
// banks.  Sweeps are in place and unsynchronised inside: every state has one owner per sweep, every value ever stored is
// the cost of a real path and values only fall, so a sweep in which no state changed (workgroup-wide OR) is the fixed
// point.  After k sweeps the k nearest states are final, so at most 8 * rows * cols sweeps are made.
template <class T>
__device__ __forceinline__ void lattice_field_body(const LatticeFieldArgs& a, T* F, int g) {
  using P = Packed<T>;
  const int rows = a.rows, cols = a.cols, stride = a.stride;
  const long long padded = a.padded, cells = (long long)rows * cols;
  const int gr = a.goals[3 * g], gc = a.goals[3 * g + 1], gh = a.goals[3 * g + 2];
  const bool goal_ok = gr >= 0 && gr < rows && gc >= 0 && gc < cols && gh >= -1 && gh < LS_HEADINGS;
  int2* out = reinterpret_cast<int2*>(a.out) + (long long)g * LS_HEADINGS * cells;
  if (!goal_ok) {   // uniform over the workgroup
    for (long long k = threadIdx.x; k < LS_HEADINGS * cells; k += LS_THREADS) out[k] = make_int2(-1, -1);
    return;
  }
  for (int h = 0; h < LS_HEADINGS; ++h) {
    const unsigned char* occ = a.occ + (long long)(h % a.layers) * cells;
    for (long long j = threadIdx.x; j < padded; j += LS_THREADS) {
      const int r = (int)(j / stride) - 1, c = (int)(j % stride) - 1;
      T v = P::WALL;
      if (r >= 0 && r < rows && c >= 0 && c < cols) {
        if (occ[(long long)r * cols + c] == 0) v = P::UNREACHED;
        if (r == gr && c == gc && (gh < 0 || gh == h)) v = 0;   // goal states are forced free
      }
      F[h * padded + j] = v;
    }
  }
  if (sizeof(T) == 8) __threadfence();
  __syncthreads();
  const long long max_sweeps = LS_HEADINGS * cells + 1;
  const T turn = (T)a.turn_cost * P::STRAIGHT;
  const int n_diag = rows + cols - 1;
  const int n_lines = 2 * rows + 2 * cols + 4 * n_diag;
  for (long long sweep = 0; sweep < max_sweeps; ++sweep) {
    int changed = 0;
    for (int q = threadIdx.x; q < n_lines; q += LS_THREADS) {
      // line q -> (heading, line of that heading): rows for h = 0, 4; columns for h = 2, 6; diagonals for odd h
      int h = 0, i = q;
      for (; h < LS_HEADINGS - 1; ++h) {
        const int n = (h & 1) ? n_diag : ((h & 2) ? cols : rows);
        if (i < n) break;
        i -= n;
      }
      const int dr = LS_DR[h], dc = LS_DC[h];
      // (r, c): the far end of the line, the cell whose straight successor is outside the image; len: its cells
      int r, c, len;
      if (dr == 0) { r = i; c = dc > 0 ? cols - 1 : 0; len = cols; }
      else if (dc == 0) { r = dr > 0 ? rows - 1 : 0; c = i; len = rows; }
      else {
        if (i < cols) { r = dr > 0 ? rows - 1 : 0; c = i; }
        else { r = i - cols + (dr > 0 ? 0 : 1); c = dc > 0 ? cols - 1 : 0; }
        const int len_r = dr > 0 ? r + 1 : rows - r, len_c = dc > 0 ? c + 1 : cols - c;
        len = len_r < len_c ? len_r : len_c;
      }
      const int hl = (h + 1) & 7, hr = (h + 7) & 7;
      T* own_p = F + h * padded;
      const T* l_p = F + hl * padded + (LS_DR[hl] * stride + LS_DC[hl]);
      const T* r_p = F + hr * padded + (LS_DR[hr] * stride + LS_DC[hr]);
      const T inc_s = (h & 1) ? P::DIAGONAL : P::STRAIGHT;
      const T inc_t = ((h & 1) ? P::STRAIGHT : P::DIAGONAL) + turn;   // h + 1 and h - 1 have the other parity
      long long j = (long long)(r + 1) * stride + c + 1;
      const int dj = -(dr * stride + dc);   // the walk goes against the heading
      T ahead = P::WALL;                    // the straight successor of the cell in hand: outside the image at the far end
      for (int k0 = 0; k0 < len; k0 += LS_BATCH) {
        T own[LS_BATCH], l[LS_BATCH], rt[LS_BATCH];
#pragma unroll
        for (int u = 0; u < LS_BATCH; ++u) {
          own[u] = l[u] = rt[u] = P::WALL;
          if (k0 + u < len) { const long long ju = j + u * dj; own[u] = own_p[ju]; l[u] = l_p[ju]; rt[u] = r_p[ju]; }
        }
#pragma unroll
        for (int u = 0; u < LS_BATCH; ++u) {
          if (k0 + u < len) {
            T v = own[u];
            if (v != P::WALL && v != 0) {
              T best = v;
              double best_k = pair_key(v);
              // the candidate's key is formed from its own pair, as the stored value's is: equal pairs have equal keys
              if (ahead < P::WALL) { const T w = ahead + inc_s; const double k = pair_key(w); if (k < best_k) { best_k = k; best = w; } }
              if (l[u] < P::WALL) { const T w = l[u] + inc_t; const double k = pair_key(w); if (k < best_k) { best_k = k; best = w; } }
              if (rt[u] < P::WALL) { const T w = rt[u] + inc_t; const double k = pair_key(w); if (k < best_k) { best_k = k; best = w; } }
              if (best != v) { own_p[j + u * dj] = best; changed = 1; v = best; }
            }
            ahead = v;
          }
        }
        j += (long long)LS_BATCH * dj;
      }
    }
    if (sizeof(T) == 8) __threadfence();   // wide path: the field lives in global memory, the next sweep must not read stale lines
    if (!__syncthreads_or(changed)) break;
  }
  for (int h = 0; h < LS_HEADINGS; ++h)
    for (long long k = threadIdx.x; k < cells; k += LS_THREADS) {
      const int r = (int)(k / cols), c = (int)(k % cols);
      const T v = F[h * padded + (long long)(r + 1) * stride + c + 1];
      out[h * cells + k] = v >= P::WALL ? make_int2(-1, -1) : make_int2(P::a(v), P::b(v));
    }
}

__global__ __launch_bounds__(LS_THREADS) void lattice_field_lds_kernel(const LatticeFieldArgs a) {
  extern __shared__ uint32_t ls_lds[];
  lattice_field_body<uint32_t>(a, ls_lds, blockIdx.x);
}

__global__ __launch_bounds__(LS_THREADS) void lattice_field_wide_kernel(const LatticeFieldArgs a) {
  lattice_field_body<uint64_t>(a, reinterpret_cast<uint64_t*>(a.work) + (long long)blockIdx.x * LS_HEADINGS * a.padded, blockIdx.x);
}

// ---- descent through the field, one problem per thread ------------------------------------------------------------------
struct LatticeTraceArgs {
  const int* fields;         // [n_fields, 8, rows, cols, 2]: fields field_first .. field_first + n_fields - 1 of n_total
  const int* start_states;   // [B, 3] (row, col, heading)
  const int* goal_states;    // [B, 3] (row, col, heading or -1)
  const int* field_index;    // [B]
  int rows, cols, turn_cost, max_len;
  long long batch, field_first, n_fields, n_total;
  int* cells;                // [B, max_len, 2]
  int* headings;             // [B, max_len]
  int* count; int* status; int* cost;
};

// successor i of heading h in the order of the rule: h, h + 1, h - 1
__device__ __forceinline__ int lattice_successor(int h, int i) { return i == 0 ? h : (i == 1 ? (h + 1) & 7 : (h + 7) & 7); }

__global__ __launch_bounds__(256) void lattice_trace_kernel(const LatticeTraceArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.batch) return;
  const int rows = a.rows, cols = a.cols, tc = a.turn_cost;
  const long long cells_n = (long long)rows * cols;
  int r = a.start_states[3 * p], c = a.start_states[3 * p + 1], h = a.start_states[3 * p + 2];
  const int gr = a.goal_states[3 * p], gc = a.goal_states[3 * p + 1];
  const long long fi = a.field_index[p];
  int status = 0, count = 0, ca = -1, cb = -1;
  if (r < 0 || r >= rows || c < 0 || c >= cols || h < 0 || h >= LS_HEADINGS || gr < 0 || gr >= rows || gc < 0 || gc >= cols ||
      fi < 0 || fi >= a.n_total) {
    status = 2;
  } else if (fi < a.field_first || fi >= a.field_first + a.n_fields) {
    return;   // the problem's field is not among the ones of this call: nothing of it is touched
  } else {
    const int2* f = reinterpret_cast<const int2*>(a.fields) + (fi - a.field_first) * LS_HEADINGS * cells_n;
    int2* cells = a.max_len > 0 ? reinterpret_cast<int2*>(a.cells) + p * a.max_len : nullptr;
    int* heads = a.max_len > 0 ? a.headings + p * a.max_len : nullptr;
    int2 d = f[h * cells_n + (long long)r * cols + c];
    int len = 0;
    if (d.x < 0) {
      double best = INFINITY;
      int bh = -1;
      for (int i = 0; i < 3; ++i) {
        const int hn = lattice_successor(h, i);
        const int nr = r + LS_DR[hn], nc = c + LS_DC[hn];
        if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
        const int2 dn = f[hn * cells_n + (long long)nr * cols + nc];
        if (dn.x < 0) continue;
        const int na = dn.x + ((hn & 1) ? 0 : 1) + (hn != h ? tc : 0), nb = dn.y + (hn & 1);
        const double k = pair_key(na, nb);   // equal pairs give equal keys: the first in order stays
        if (k < best) { best = k; bh = hn; ca = na; cb = nb; }
      }
      if (bh < 0) status = 1;
      else {
        if (cells && len < a.max_len) { cells[len] = make_int2(r, c); heads[len] = h; }
        ++len;
        r += LS_DR[bh]; c += LS_DC[bh]; h = bh;
        d = f[h * cells_n + (long long)r * cols + c];
      }
    } else {
      ca = d.x; cb = d.y;
    }
    if (status == 0) {
      // every move lowers a + b by at least one, so the walk ends; the bound keeps a field that is no fixed point finite
      const long long max_steps = LS_HEADINGS * cells_n;
      for (long long step = 0;; ++step) {
        if (cells && len < a.max_len) { cells[len] = make_int2(r, c); heads[len] = h; }
        ++len;
        if ((d.x == 0 && d.y == 0) || step >= max_steps) break;
        int pick = -1;
        int2 dn = d;
        for (int i = 0; i < 3 && pick < 0; ++i) {
          const int hn = lattice_successor(h, i);
          const int nr = r + LS_DR[hn], nc = c + LS_DC[hn];
          if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
          dn = f[hn * cells_n + (long long)nr * cols + nc];
          if (dn.x >= 0 && dn.x + ((hn & 1) ? 0 : 1) + (hn != h ? tc : 0) == d.x && dn.y + (hn & 1) == d.y) pick = hn;
        }
        if (pick < 0) break;   // cannot happen on a fixed-point field
        r += LS_DR[pick]; c += LS_DC[pick]; h = pick;
        d = dn;
      }
      count = len;
    } else {
      ca = cb = -1;
    }
  }
  a.count[p] = count;
  a.status[p] = status;
  if (a.cost) { a.cost[2 * p] = ca; a.cost[2 * p + 1] = cb; }
}

// -> false: refused.  *lds: the packed form in LDS applies.
static bool lattice_shape(int rows, int cols, int turn_cost, int* stride, long long* padded, bool* lds) {
  if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768 || turn_cost < 0 || turn_cost > 255) return false;
  const long long counts = (long long)LS_HEADINGS * rows * cols * (1 + turn_cost);
  if (counts >= LS_MAX_COUNT) return false;
  *stride = (cols + 2) | 1;   // odd: lines a row apart fall on different LDS banks
  *padded = (long long)(rows + 2) * *stride;
  *lds = LS_HEADINGS * *padded <= LS_LDS_WORDS && counts <= 65535;   // no 16-bit count can wrap
  return true;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_lattice_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int64_t n_goals) {
  int stride;
  long long padded;
  bool lds;
  if (n_goals < 1 || !lattice_shape(rows, cols, turn_cost, &stride, &padded, &lds) || lds) return 0;
  return (size_t)padded * LS_HEADINGS * 8 * (size_t)n_goals;
}

extern "C" int nfopp_lattice_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                             const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost,
                                             int32_t* fields_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768, "grid must be 1..32768 cells a side");
  NFOPP_REQUIRE(n_layers == 1 || n_layers == 8, "occupancy must have 1 or 8 layers, not %d", n_layers);
  NFOPP_REQUIRE(turn_cost >= 0 && turn_cost <= 255, "turn_cost must be 0..255, not %d", turn_cost);
  LatticeFieldArgs a;
  bool lds;
  NFOPP_REQUIRE(lattice_shape(rows, cols, turn_cost, &a.stride, &a.padded, &lds),
                "8 * rows * cols * (1 + turn_cost) reaches 2^21: path counts could leave the exactly ordered range");
  NFOPP_REQUIRE(n_goals >= 0 && n_goals <= 0x7fffffffLL, "bad goal count");
  if (n_goals == 0) return NFOPP_OK;
  NFOPP_REQUIRE(layers_dev && goal_states_dev && fields_dev, "null device pointer");
  a.occ = layers_dev; a.goals = goal_states_dev; a.layers = n_layers; a.rows = rows; a.cols = cols; a.turn_cost = turn_cost;
  a.out = fields_dev; a.work = nullptr;
  if (lds) {
    static bool attr_set[MAX_DEVICES] = {};
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(lattice_field_lds_kernel), (size_t)LS_LDS_WORDS * 4, attr_set);
    if (rc != NFOPP_OK) return rc;
    hipLaunchKernelGGL(lattice_field_lds_kernel, dim3((unsigned)n_goals), dim3(LS_THREADS), (size_t)a.padded * LS_HEADINGS * 4,
                       (hipStream_t)stream, a);
  } else {
    const size_t need = (size_t)a.padded * LS_HEADINGS * 8 * (size_t)n_goals;
    NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small: nfopp_lattice_fields_workspace_bytes gives %zu", need);
    NFOPP_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace must be 8-byte aligned");
    a.work = workspace_dev;
    hipLaunchKernelGGL(lattice_field_wide_kernel, dim3((unsigned)n_goals), dim3(LS_THREADS), 0, (hipStream_t)stream, a);
  }
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_lattice_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                                         int32_t rows, int32_t cols, int32_t turn_cost, const int32_t* start_states_dev,
                                         const int32_t* goal_states_dev, const int32_t* field_index_dev, int64_t batch,
                                         int32_t max_len, int32_t* cells_dev, int32_t* headings_dev, int32_t* count_dev,
                                         int32_t* status_dev, int32_t* cost_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && max_len >= 0, "bad sizes");
  NFOPP_REQUIRE((long long)LS_HEADINGS * rows * cols < LS_MAX_COUNT, "grid beyond the limit of nfopp_lattice_distance_fields");
  NFOPP_REQUIRE(turn_cost >= 0 && turn_cost <= 255, "turn_cost must be 0..255, not %d", turn_cost);
  NFOPP_REQUIRE(field_first >= 0 && n_fields >= 0 && n_total >= 0 && field_first + n_fields <= n_total, "bad field range");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL, "bad batch");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(start_states_dev && goal_states_dev && field_index_dev && count_dev && status_dev, "null device pointer");
  NFOPP_REQUIRE((fields_dev || n_fields == 0) && ((cells_dev && headings_dev) || max_len == 0), "null device pointer");
  LatticeTraceArgs a;
  a.fields = fields_dev; a.start_states = start_states_dev; a.goal_states = goal_states_dev; a.field_index = field_index_dev;
  a.rows = rows; a.cols = cols; a.turn_cost = turn_cost; a.max_len = max_len; a.batch = batch;
  a.field_first = field_first; a.n_fields = n_fields; a.n_total = n_total;
  a.cells = cells_dev; a.headings = headings_dev; a.count = count_dev; a.status = status_dev; a.cost = cost_dev;
  hipLaunchKernelGGL(lattice_trace_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
