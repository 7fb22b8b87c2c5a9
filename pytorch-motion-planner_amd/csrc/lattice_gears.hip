// Lattice search with reverse moves and gear changes: cost-to-goal fields over (cell, heading, gear) states and a descent
// through them per problem that reports the gear of every move.  The traced cells and headings go through
// nfopp_lattice_seed_trajectories (grid_search.hip), which takes the body heading from the lattice states.  The rule is this
// library's own (the reference has no such search); it is stated here, in include/nfopp_hip.h and in
// tests/lattice_gears_ref.py.  What it shares with lattice_search.hip is lattice_field.h's; the relaxation and the trace's
// start rule and walk are here.
//
// STATE.  (cell c = (row, col), heading h in 0 .. 7, gear s in {0 forward, 1 reverse}); heading h stands for the angle
//   h * pi / 4; s is the gear of the move that entered the state.  Occupancy does not depend on s.
// DIRECTIONS, OCCUPANCY, STATUS.  As in lattice_search.hip's rule; dir(h) is the table of lattice_field.h, and state
//   (c, h, s) reads occupancy layer h mod L.
// MOVES.  Forward, gear 0: from (c, h) to (c + dir(h'), h').  Reverse, gear 1: from (c, h) to (c - dir(h), h') -- a forward
//   move run backwards in time, so the robot backs along the heading it had BEFORE the move.  In both h' in {h, h + 1, h - 1}
//   mod 8, and the target state must be free.
// COST.  An integer pair (a, b) ordered exactly as a + b * sqrt 2 (pair_cost.h).  A forward move adds (1, 0) for even h' and
//   (0, 1) for odd h'; a reverse move adds (1, 0) for even h and (0, 1) for odd h: the parity of the direction it moves
//   along.  Either adds (turn_cost, 0) where h' != h; a reverse move adds a further (reverse_cost, 0); a move whose gear
//   differs from s adds (cusp_cost, 0).  The three costs are integers 0 .. 255.  Equal cost means equal pair, so the field is
//   the unique fixed point of the relaxation and is compared with ==.
// GOAL.  (goal cell, goal heading or -1) as there, at both gears: cost (0, 0), forced free.
// FIELD.  d_g(s, h, c) = the minimum cost from (c, h, s) to g, int32 [G, 2, 8, rows, cols, 2]; the sentinel as there.
// TRACE.  Problem p starts in (start cell, start heading).  The start has no gear: its first move is charged no cusp cost.
//   The start state is NOT tested for occupancy.  A start that is a goal state gives the one-state path with cost (0, 0).
//   Otherwise the first move is the one of the six successors with the smallest d(successor) + move cost without the cusp
//   term; the order is forward h, h + 1, h - 1, then reverse h, h + 1, h - 1, ties go to the first in that order; the path's
//   cost is that sum; if no successor has a cost the status is 1.  After the first move the next state is the first
//   successor in the same order whose cost plus the move (with the cusp term) equals the current cost exactly; the trace
//   ends at the first state with cost (0, 0).  This one rule covers blocked starts too.
// OUTPUTS.  cells [B, max_len, 2], headings [B, max_len], gears [B, max_len], count, status, cost.  gears[k] is the gear of
//   the move into state k; gears[0] is the gear of the first move, or 0 for a one-state path.
// REFUSED before launch, nothing is clamped: a cost outside 0 .. 255, L not 1 or 8, 16 * rows * cols * (1 + turn_cost +
//   reverse_cost + cusp_cost) >= 2^21 (the bound under which the float64 key orders pairs exactly, on the largest count a
//   path over 16 * rows * cols states can reach), a short or misaligned workspace, null required pointers.
#include "common.h"
#include "lattice_field.h"
#include "pair_cost.h"

namespace nfopp {

constexpr int LG_STATES = 2 * LATTICE_HEADINGS;   // layers of a field: gear * 8 + heading
constexpr int LG_BATCH = 2;   // cells of a line a thread has in flight: their 7 reads each are issued before any is used

// the smaller of (best, w) by the pair order; the candidate's key is formed from its own pair, as the stored value's is, so
// equal pairs have equal keys and the first stays
template <class T>
__device__ __forceinline__ void gear_take(T w, T& best, double& best_k) {
  const double k = pair_key(w);
  if (k < best_k) { best_k = k; best = w; }
}

// The field frame of lattice_field.h with 16 layers, gear * 8 + heading.  The goal decode, the fill and the line map below are
// this file's own text, the same as lattice_goal, lattice_fill_layer and lattice_line of the header (the line map pinned
// equal by tests/test_lattice_gears_cpu.py): called as helpers, each moved the scheduling of these two kernels and with it
// their time beyond the parent's run-to-run spread (profiles/lattice_field.txt); the store and n_lines did not.
// A thread owns both gears of its line's cells and walks the line twice a sweep.  Pass 1 goes against the heading from the
// far end and carries d(0, h, .) of the cell ahead in a register, so a straight forward run of any length settles in one
// sweep; pass 2 goes with the heading from the near end and carries
// d(1, h, .) of the cell behind, so a straight reverse run does.  At a cell both passes form
//   FW = min over h' of d(0, h', c + dir(h')) + length(h') + turn,   RV = min over h' of d(1, h', c - dir(h)) + length(h) + turn
//        + reverse_cost
// and lower d(0, h, c) to min(FW, RV + cusp) and d(1, h, c) to min(FW + cusp, RV): seven reads and the carried value for
// two states, the reads of LG_BATCH cells issued before the arithmetic of the first.  The turning reverse successors sit
// at the neighbouring cell c - dir(h), not in place.  At most 16 * rows * cols sweeps are made.
template <class T>
__device__ __forceinline__ void gear_field_body(const LatticeFieldArgs& a, T* F, int g) {
  using P = Packed<T>;
  const int rows = a.rows, cols = a.cols, stride = a.stride;
  const long long padded = a.padded, cells = (long long)rows * cols;
  const int gr = a.goals[3 * g], gc = a.goals[3 * g + 1], gh = a.goals[3 * g + 2];
  const bool goal_ok = gr >= 0 && gr < rows && gc >= 0 && gc < cols && gh >= -1 && gh < LATTICE_HEADINGS;
  int2* out = reinterpret_cast<int2*>(a.out) + (long long)g * LG_STATES * cells;
  if (!goal_ok) {   // uniform over the workgroup
    for (long long k = threadIdx.x; k < LG_STATES * cells; k += LATTICE_THREADS) out[k] = make_int2(-1, -1);
    return;
  }
  for (int h = 0; h < LATTICE_HEADINGS; ++h) {
    const unsigned char* occ = a.occ + (long long)(h % a.layers) * cells;
    for (long long j = threadIdx.x; j < padded; j += LATTICE_THREADS) {
      const int r = (int)(j / stride) - 1, c = (int)(j % stride) - 1;
      T v = P::WALL;
      if (r >= 0 && r < rows && c >= 0 && c < cols) {
        if (occ[(long long)r * cols + c] == 0) v = P::UNREACHED;
        if (r == gr && c == gc && (gh < 0 || gh == h)) v = 0;   // goal states are forced free, at both gears
      }
      F[h * padded + j] = v;
      F[(LATTICE_HEADINGS + h) * padded + j] = v;
    }
  }
  if (sizeof(T) == 8) __threadfence();
  __syncthreads();
  const long long max_sweeps = LG_STATES * cells + 1;
  const T turn = (T)a.turn_cost * P::STRAIGHT;
  const T rev = (T)a.reverse_cost * P::STRAIGHT;
  const T cusp = (T)a.cusp_cost * P::STRAIGHT;
  const int n_diag = rows + cols - 1;
  const int n_lines = lattice_n_lines(rows, cols);
  for (long long sweep = 0; sweep < max_sweeps; ++sweep) {
    int changed = 0;
    for (int q = threadIdx.x; q < n_lines; q += LATTICE_THREADS) {
      int h = 0, i = q;
      for (; h < LATTICE_HEADINGS - 1; ++h) {
        const int n = (h & 1) ? n_diag : ((h & 2) ? cols : rows);
        if (i < n) break;
        i -= n;
      }
      const int dr = LATTICE_DR[h], dc = LATTICE_DC[h];
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
      const int step = dr * stride + dc;                       // one cell along the heading
      T* own0 = F + h * padded;
      T* own1 = F + (LATTICE_HEADINGS + h) * padded;
      const T* fl_p = F + hl * padded + (LATTICE_DR[hl] * stride + LATTICE_DC[hl]);   // forward turn successors: gear 0, c + dir(h')
      const T* fr_p = F + hr * padded + (LATTICE_DR[hr] * stride + LATTICE_DC[hr]);
      const T* bl_p = F + (LATTICE_HEADINGS + hl) * padded - step;               // reverse turn successors: gear 1, c - dir(h)
      const T* br_p = F + (LATTICE_HEADINGS + hr) * padded - step;
      const T inc_s = (h & 1) ? P::DIAGONAL : P::STRAIGHT;                  // along dir(h): forward straight, every reverse move
      const T inc_ft = ((h & 1) ? P::STRAIGHT : P::DIAGONAL) + turn;        // h + 1 and h - 1 have the other parity
      const T inc_rs = inc_s + rev, inc_rt = inc_s + rev + turn;
      const long long j_far = (long long)(r + 1) * stride + c + 1;
      for (int pass = 0; pass < 2; ++pass) {
        // pass 0: from the far end against the heading, `carry` = d(0, h, c + dir(h)); pass 1: from the near end with the
        // heading, `carry` = d(1, h, c - dir(h)).  Beyond either end lies the blocked border.
        long long jb = pass == 0 ? j_far : j_far - (long long)(len - 1) * step;
        const int dj = pass == 0 ? -step : step;
        T carry = P::WALL;
        // the other straight successor, not carried: pass 0 reads d(1, h, c - dir(h)), pass 1 reads d(0, h, c + dir(h)); both lie
        // one cell further along the walk, so this pass has not touched them yet
        const T* next_p = pass == 0 ? own1 - step : own0 + step;
        for (int k0 = 0; k0 < len; k0 += LG_BATCH) {
          T o0[LG_BATCH], o1[LG_BATCH], nx[LG_BATCH], tfl[LG_BATCH], tfr[LG_BATCH], tbl[LG_BATCH], tbr[LG_BATCH];
#pragma unroll
          for (int u = 0; u < LG_BATCH; ++u) {   // the reads of LG_BATCH cells are issued before any is used
            o0[u] = o1[u] = nx[u] = tfl[u] = tfr[u] = tbl[u] = tbr[u] = P::WALL;
            if (k0 + u < len) {
              const long long ju = jb + u * dj;
              o0[u] = own0[ju]; o1[u] = own1[ju]; nx[u] = next_p[ju];
              tfl[u] = fl_p[ju]; tfr[u] = fr_p[ju]; tbl[u] = bl_p[ju]; tbr[u] = br_p[ju];
            }
          }
#pragma unroll
          for (int u = 0; u < LG_BATCH; ++u) {
            if (k0 + u >= len) break;
            T v0 = o0[u], v1 = o1[u];
            const T ahead = pass == 0 ? carry : nx[u];
            const T behind = pass == 0 ? nx[u] : carry;
            const T fl = tfl[u], fr = tfr[u], bl = tbl[u], br = tbr[u];
            const long long j = jb + u * dj;
            if (v0 != P::WALL && v0 != 0) {   // occupancy and the goal are the same at both gears
              T fw = P::UNREACHED, rv = P::UNREACHED;
              double fw_k = INFINITY, rv_k = INFINITY;
              if (ahead < P::WALL) gear_take<T>(ahead + inc_s, fw, fw_k);
              if (fl < P::WALL) gear_take<T>(fl + inc_ft, fw, fw_k);
              if (fr < P::WALL) gear_take<T>(fr + inc_ft, fw, fw_k);
              if (behind < P::WALL) gear_take<T>(behind + inc_rs, rv, rv_k);
              if (bl < P::WALL) gear_take<T>(bl + inc_rt, rv, rv_k);
              if (br < P::WALL) gear_take<T>(br + inc_rt, rv, rv_k);
              T b0 = v0, b1 = v1;
              double b0_k = pair_key(v0), b1_k = pair_key(v1);
              if (fw < P::WALL) { gear_take<T>(fw, b0, b0_k); gear_take<T>(fw + cusp, b1, b1_k); }
              if (rv < P::WALL) { gear_take<T>(rv + cusp, b0, b0_k); gear_take<T>(rv, b1, b1_k); }
              if (b0 != v0) { own0[j] = b0; changed = 1; v0 = b0; }
              if (b1 != v1) { own1[j] = b1; changed = 1; v1 = b1; }
            }
            carry = pass == 0 ? v0 : v1;
          }
          jb += (long long)LG_BATCH * dj;
        }
      }
    }
    if (sizeof(T) == 8) __threadfence();   // wide path: the field lives in global memory, the next sweep must not read stale lines
    if (!__syncthreads_or(changed)) break;
  }
  for (int l = 0; l < LG_STATES; ++l) lattice_store_layer<T, LATTICE_THREADS>(F, l * padded, out, l * cells, cells, cols, stride);
}

__global__ __launch_bounds__(LATTICE_THREADS) void gear_field_lds_kernel(const LatticeFieldArgs a) {
  extern __shared__ uint32_t lg_lds[];
  gear_field_body<uint32_t>(a, lg_lds, blockIdx.x);
}

__global__ __launch_bounds__(LATTICE_THREADS) void gear_field_wide_kernel(const LatticeFieldArgs a) {
  gear_field_body<uint64_t>(a, reinterpret_cast<uint64_t*>(a.work) + (long long)blockIdx.x * LG_STATES * a.padded, blockIdx.x);
}

// ---- descent through the field, one problem per thread ------------------------------------------------------------------
// the start rule and the walk of the search with gears: all six successors of lattice_successor
__global__ __launch_bounds__(256) void gear_trace_kernel(const LatticeTraceArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.batch) return;
  const int rows = a.rows, cols = a.cols, tc = a.turn_cost, rc = a.reverse_cost, cc = a.cusp_cost;
  const long long cells_n = (long long)rows * cols;
  int r, c, h;
  const int2* f;
  int status = lattice_trace_begin(a, p, LG_STATES, &r, &c, &h, &f);
  if (status < 0) return;
  int len = 0, ca = -1, cb = -1;
  if (status == 0) {
    int2* cells = a.max_len > 0 ? reinterpret_cast<int2*>(a.cells) + p * a.max_len : nullptr;
    int* heads = a.max_len > 0 ? a.headings + p * a.max_len : nullptr;
    int* gears = a.max_len > 0 ? a.gears + p * a.max_len : nullptr;
    int2 d = f[h * cells_n + (long long)r * cols + c];   // goal states hold (0, 0) at both gears, and only they do
    int s = 0;
    if (d.x == 0 && d.y == 0) {
      if (cells) { lattice_record(cells, heads, 0, r, c, h); gears[0] = 0; }
      len = 1; ca = cb = 0;
    } else {
      double best = INFINITY;
      int bi = -1;
      for (int i = 0; i < 6; ++i) {
        int nr, nc, nh, ns, ma, mb;
        if (!lattice_successor(r, c, h, i, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
        const int2 dn = f[(ns * LATTICE_HEADINGS + nh) * cells_n + (long long)nr * cols + nc];
        if (dn.x < 0) continue;
        const double k = pair_key(dn.x + ma, dn.y + mb);   // equal pairs give equal keys: the first in order stays
        if (k < best) { best = k; bi = i; ca = dn.x + ma; cb = dn.y + mb; }
      }
      if (bi < 0) status = 1;
      else {
        int nr, nc, nh, ns, ma, mb;
        lattice_successor(r, c, h, bi, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb);
        if (cells) { lattice_record(cells, heads, 0, r, c, h); gears[0] = ns; }
        len = 1;
        r = nr; c = nc; h = nh; s = ns;
        d = f[(s * LATTICE_HEADINGS + h) * cells_n + (long long)r * cols + c];
        // every move lowers a + b by at least one, so the walk ends; the bound keeps a field that is no fixed point finite
        const long long max_steps = LG_STATES * cells_n;
        for (long long step = 0;; ++step) {
          if (cells && len < a.max_len) { lattice_record(cells, heads, len, r, c, h); gears[len] = s; }
          ++len;
          if ((d.x == 0 && d.y == 0) || step >= max_steps) break;
          int pick = -1;
          int2 dn = d;
          for (int i = 0; i < 6 && pick < 0; ++i) {
            if (!lattice_successor(r, c, h, i, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
            dn = f[(ns * LATTICE_HEADINGS + nh) * cells_n + (long long)nr * cols + nc];
            if (dn.x >= 0 && dn.x + ma + (ns != s ? cc : 0) == d.x && dn.y + mb == d.y) pick = i;
          }
          if (pick < 0) break;   // cannot happen on a fixed-point field
          r = nr; c = nc; h = nh; s = ns;
          d = dn;
        }
        if (d.x != 0 || d.y != 0) status = 1;   // a caller's field that is no fixed point: the walk did not reach the goal
      }
    }
  }
  lattice_trace_end(a.count, a.status, a.cost, p, len, status, ca, cb);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_lattice_gear_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost,
                                                            int32_t cusp_cost, int64_t n_goals) {
  return lattice_workspace_bytes(rows, cols, LG_STATES, lattice_cost_sum(turn_cost, reverse_cost, cusp_cost), n_goals);
}

extern "C" int nfopp_lattice_gear_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                                  const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost,
                                                  int32_t reverse_cost, int32_t cusp_cost, int32_t* fields_dev,
                                                  void* workspace_dev, size_t workspace_bytes, void* stream) {
  return lattice_fields_entry<gear_field_lds_kernel, gear_field_wide_kernel>(
      layers_dev, n_layers, rows, cols, goal_states_dev, n_goals,
      {{"turn_cost", turn_cost}, {"reverse_cost", reverse_cost}, {"cusp_cost", cusp_cost}}, fields_dev, workspace_dev, workspace_bytes,
      stream, LG_STATES,
      "16 * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost) reaches 2^21: path counts could leave the exactly ordered range",
      "workspace too small: nfopp_lattice_gear_fields_workspace_bytes gives %zu");
}

extern "C" int nfopp_lattice_gear_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                                              int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost,
                                              int32_t cusp_cost, const int32_t* start_states_dev, const int32_t* goal_states_dev,
                                              const int32_t* field_index_dev, int64_t batch, int32_t max_len, int32_t* cells_dev,
                                              int32_t* headings_dev, int32_t* gears_dev, int32_t* count_dev, int32_t* status_dev,
                                              int32_t* cost_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768 && max_len >= 0, "bad sizes");
  LATTICE_REQUIRE_COST(turn_cost);
  LATTICE_REQUIRE_COST(reverse_cost);
  LATTICE_REQUIRE_COST(cusp_cost);
  NFOPP_REQUIRE(lattice_cost_sum(turn_cost, reverse_cost, cusp_cost) * LG_STATES * rows * cols < LATTICE_MAX_COUNT,
                "grid and costs beyond the limit of nfopp_lattice_gear_distance_fields");
  const LatticeTraceArgs a = {fields_dev, start_states_dev, goal_states_dev, field_index_dev, rows, cols, turn_cost, reverse_cost,
                              cusp_cost, max_len, batch, field_first, n_fields, n_total, cells_dev, headings_dev, gears_dev, count_dev,
                              status_dev, cost_dev};
  return lattice_trace_launch<gear_trace_kernel>(a, cells_dev && headings_dev && gears_dev, stream);
}
