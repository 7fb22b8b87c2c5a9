// Heading-aware lattice search for car-like trajectory seeds: cost-to-goal fields over (cell, heading) states and a
// descent through them per problem.  The traced cells go through nfopp_grid_seed_trajectories unchanged.  The rule is this
// library's own (the reference has no such search); it is stated here, in include/nfopp_hip.h and in tests/lattice_ref.py.
// What it shares with lattice_gears.hip is lattice_field.h's; the relaxation and the trace's start rule and walk are here.
//
// STATE.  (cell (row, col), heading h in 0 .. 7); heading h stands for the angle h * pi / 4.
// DIRECTIONS.  dir(h) as (d row, d col): the table of lattice_field.h.
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
#include "lattice_field.h"
#include "pair_cost.h"

namespace nfopp {

constexpr int LS_STATES = LATTICE_HEADINGS;   // layers of a field: one per heading
constexpr int LS_BATCH = 4;   // cells of a line a thread has in flight: their 3 reads each are issued before any is used

// The field frame of lattice_field.h with 8 layers, one per heading.  A thread walks its line of layer h against the heading
// from the far end, the straight successor's value carried in a register: a straight run of any length settles in ONE
// sweep, so the sweeps a field needs follow the turns of its paths, not their lengths.  Per cell the walk reads the state
// itself and the two turn successors (layers h + 1 and h - 1), LS_BATCH cells ahead of the arithmetic.  At most
// 8 * rows * cols sweeps are made.
template <class T>
__device__ __forceinline__ void lattice_field_body(const LatticeFieldArgs& a, T* F, int g) {
  using P = Packed<T>;
  const int rows = a.rows, cols = a.cols, stride = a.stride;
  const long long padded = a.padded, cells = (long long)rows * cols;
  int gr, gc, gh;
  int2* out = reinterpret_cast<int2*>(a.out) + (long long)g * LS_STATES * cells;
  // uniform over the workgroup
  if (!lattice_goal<LATTICE_THREADS>(a.goals, g, rows, cols, &gr, &gc, &gh, out, LS_STATES * cells)) return;
  for (int h = 0; h < LATTICE_HEADINGS; ++h)
    lattice_fill_layer<T, LATTICE_THREADS>(F + h * padded, a.occ + (long long)(h % a.layers) * cells, rows, cols, stride, padded, gr,
                                           gc, gh < 0 || gh == h);
  if (sizeof(T) == 8) __threadfence();
  __syncthreads();
  const long long max_sweeps = LS_STATES * cells + 1;
  const T turn = (T)a.turn_cost * P::STRAIGHT;
  const int n_lines = lattice_n_lines(rows, cols);
  for (long long sweep = 0; sweep < max_sweeps; ++sweep) {
    int changed = 0;
    for (int q = threadIdx.x; q < n_lines; q += LATTICE_THREADS) {
      const LatticeLine line = lattice_line(q, rows, cols, stride);
      const int h = line.h, len = line.len;
      const int hl = (h + 1) & 7, hr = (h + 7) & 7;
      T* own_p = F + h * padded;
      const T* l_p = F + hl * padded + (LATTICE_DR[hl] * stride + LATTICE_DC[hl]);
      const T* r_p = F + hr * padded + (LATTICE_DR[hr] * stride + LATTICE_DC[hr]);
      const T inc_s = (h & 1) ? P::DIAGONAL : P::STRAIGHT;
      const T inc_t = ((h & 1) ? P::STRAIGHT : P::DIAGONAL) + turn;   // h + 1 and h - 1 have the other parity
      long long j = line.far;
      const int dj = -line.step;   // the walk goes against the heading
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
  for (int l = 0; l < LS_STATES; ++l) lattice_store_layer<T, LATTICE_THREADS>(F, l * padded, out, l * cells, cells, cols, stride);
}

__global__ __launch_bounds__(LATTICE_THREADS) void lattice_field_lds_kernel(const LatticeFieldArgs a) {
  extern __shared__ uint32_t ls_lds[];
  lattice_field_body<uint32_t>(a, ls_lds, blockIdx.x);
}

__global__ __launch_bounds__(LATTICE_THREADS) void lattice_field_wide_kernel(const LatticeFieldArgs a) {
  lattice_field_body<uint64_t>(a, reinterpret_cast<uint64_t*>(a.work) + (long long)blockIdx.x * LS_STATES * a.padded, blockIdx.x);
}

// ---- descent through the field, one problem per thread ------------------------------------------------------------------
// the start rule and the walk of the forward-only search: successors i < 3 of lattice_successor, no reverse cost
__global__ __launch_bounds__(256) void lattice_trace_kernel(const LatticeTraceArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.batch) return;
  const int rows = a.rows, cols = a.cols, tc = a.turn_cost;
  const long long cells_n = (long long)rows * cols;
  int r, c, h, nr, nc, nh, ns, ma, mb;
  const int2* f;
  int status = lattice_trace_begin(a, p, LS_STATES, &r, &c, &h, &f);
  if (status < 0) return;
  int len = 0, ca = -1, cb = -1;
  if (status == 0) {
    int2* cells = a.max_len > 0 ? reinterpret_cast<int2*>(a.cells) + p * a.max_len : nullptr;
    int* heads = a.max_len > 0 ? a.headings + p * a.max_len : nullptr;
    int2 d = f[h * cells_n + (long long)r * cols + c];
    if (d.x < 0) {   // a blocked start: the first step goes to the successor with the smallest d + move
      double best = INFINITY;
      int bi = -1;
      for (int i = 0; i < 3; ++i) {
        if (!lattice_successor(r, c, h, i, rows, cols, tc, 0, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
        const int2 dn = f[nh * cells_n + (long long)nr * cols + nc];
        if (dn.x < 0) continue;
        const double k = pair_key(dn.x + ma, dn.y + mb);   // equal pairs give equal keys: the first in order stays
        if (k < best) { best = k; bi = i; ca = dn.x + ma; cb = dn.y + mb; }
      }
      if (bi < 0) status = 1;
      else {
        if (cells && len < a.max_len) lattice_record(cells, heads, len, r, c, h);
        ++len;
        lattice_successor(r, c, h, bi, rows, cols, tc, 0, &nr, &nc, &nh, &ns, &ma, &mb);
        r = nr; c = nc; h = nh;
        d = f[h * cells_n + (long long)r * cols + c];
      }
    } else {
      ca = d.x; cb = d.y;
    }
    if (status == 0) {
      // every move lowers a + b by at least one, so the walk ends; the bound keeps a field that is no fixed point finite
      const long long max_steps = LS_STATES * cells_n;
      for (long long step = 0;; ++step) {
        if (cells && len < a.max_len) lattice_record(cells, heads, len, r, c, h);
        ++len;
        if ((d.x == 0 && d.y == 0) || step >= max_steps) break;
        int pick = -1;
        int2 dn = d;
        for (int i = 0; i < 3 && pick < 0; ++i) {
          if (!lattice_successor(r, c, h, i, rows, cols, tc, 0, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
          dn = f[nh * cells_n + (long long)nr * cols + nc];
          if (dn.x >= 0 && dn.x + ma == d.x && dn.y + mb == d.y) pick = i;
        }
        if (pick < 0) break;   // cannot happen on a fixed-point field
        r = nr; c = nc; h = nh;
        d = dn;
      }
    }
  }
  lattice_trace_end(a.count, a.status, a.cost, p, len, status, ca, cb);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_lattice_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int64_t n_goals) {
  return lattice_workspace_bytes(rows, cols, LS_STATES, lattice_cost_sum(turn_cost), n_goals);
}

extern "C" int nfopp_lattice_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                             const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost,
                                             int32_t* fields_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return lattice_fields_entry<lattice_field_lds_kernel, lattice_field_wide_kernel>(
      layers_dev, n_layers, rows, cols, goal_states_dev, n_goals, {{"turn_cost", turn_cost}}, fields_dev, workspace_dev, workspace_bytes,
      stream, LS_STATES, "8 * rows * cols * (1 + turn_cost) reaches 2^21: path counts could leave the exactly ordered range",
      "workspace too small: nfopp_lattice_fields_workspace_bytes gives %zu");
}

extern "C" int nfopp_lattice_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                                         int32_t rows, int32_t cols, int32_t turn_cost, const int32_t* start_states_dev,
                                         const int32_t* goal_states_dev, const int32_t* field_index_dev, int64_t batch,
                                         int32_t max_len, int32_t* cells_dev, int32_t* headings_dev, int32_t* count_dev,
                                         int32_t* status_dev, int32_t* cost_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && max_len >= 0, "bad sizes");   // no rows <= 32768 test here; the gear trace has one
  // the bound leaves out the (1 + turn_cost) factor that the field entry and the gear trace apply
  NFOPP_REQUIRE((long long)LS_STATES * rows * cols < LATTICE_MAX_COUNT, "grid beyond the limit of nfopp_lattice_distance_fields");
  LATTICE_REQUIRE_COST(turn_cost);
  const LatticeTraceArgs a = {fields_dev, start_states_dev, goal_states_dev, field_index_dev, rows, cols, turn_cost, 0, 0, max_len,
                              batch, field_first, n_fields, n_total, cells_dev, headings_dev, nullptr, count_dev, status_dev, cost_dev};
  return lattice_trace_launch<lattice_trace_kernel>(a, cells_dev && headings_dev, stream);
}
