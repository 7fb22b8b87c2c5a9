// Lattice search with reverse moves and gear changes: cost-to-goal fields over (cell, heading, gear) states and a descent
// through them per problem that reports the gear of every move.  The traced cells and headings go through
// nfopp_lattice_seed_trajectories (grid_search.hip), which takes the body heading from the lattice states.  The rule is this
// library's own (the reference has no such search); it is stated here, in include/nfopp_hip.h and in
// tests/lattice_gears_ref.py.  Directions, headings, occupancy layers and the pair order are lattice_search.hip's.
//
// STATE.  (cell c = (row, col), heading h in 0 .. 7, gear s in {0 forward, 1 reverse}); heading h stands for the angle
//   h * pi / 4; s is the gear of the move that entered the state.  Occupancy does not depend on s.
// DIRECTIONS.  dir(h) as (d row, d col), row = y and col = x as in the occupancy grid:
//   h      0       1       2       3       4        5        6       7
//   dir  (0,+1)  (+1,+1)  (+1,0)  (+1,-1)  (0,-1)  (-1,-1)  (-1,0)  (-1,+1)
// OCCUPANCY.  layers uint8 [L, rows, cols], L = 1 or 8, non-zero = blocked; state (c, h, s) reads layer h mod L; cells
//   outside the image are blocked; no corner rule between states.
// MOVES.  Forward, gear 0: from (c, h) to (c + dir(h'), h').  Reverse, gear 1: from (c, h) to (c - dir(h), h') -- a forward
//   move run backwards in time, so the robot backs along the heading it had BEFORE the move.  In both h' in {h, h + 1, h - 1}
//   mod 8, and the target state must be free.
// COST.  An integer pair (a, b) ordered exactly as a + b * sqrt 2 (pair_cost.h).  A forward move adds (1, 0) for even h' and
//   (0, 1) for odd h'; a reverse move adds (1, 0) for even h and (0, 1) for odd h: the parity of the direction it moves
//   along.  Either adds (turn_cost, 0) where h' != h; a reverse move adds a further (reverse_cost, 0); a move whose gear
//   differs from s adds (cusp_cost, 0).  The three costs are integers 0 .. 255.  Equal cost means equal pair, so the field is
//   the unique fixed point of the relaxation and is compared with ==.
// GOAL.  (goal cell, goal heading) at both gears; with goal heading -1 the goal cell at every heading.  Goal states have cost
//   (0, 0) and are forced free.
// FIELD.  d_g(s, h, c) = the minimum cost from (c, h, s) to g, int32 [G, 2, 8, rows, cols, 2].  The sentinel (-1, -1) marks
//   blocked states, states that cannot reach g, and every state of a goal whose cell is outside the grid or whose heading is
//   outside -1 .. 7.
// TRACE.  Problem p starts in (start cell, start heading).  The start has no gear: its first move is charged no cusp cost.
//   The start state is NOT tested for occupancy.  A start that is a goal state gives the one-state path with cost (0, 0).
//   Otherwise the first move is the one of the six successors with the smallest d(successor) + move cost without the cusp
//   term; the order is forward h, h + 1, h - 1, then reverse h, h + 1, h - 1, ties go to the first in that order; the path's
//   cost is that sum; if no successor has a cost the status is 1.  After the first move the next state is the first
//   successor in the same order whose cost plus the move (with the cusp term) equals the current cost exactly; the trace
//   ends at the first state with cost (0, 0).  This one rule covers blocked starts too.
// OUTPUTS.  cells [B, max_len, 2], headings [B, max_len], gears [B, max_len], count, status, cost.  gears[k] is the gear of
//   the move into state k; gears[0] is the gear of the first move, or 0 for a one-state path.
// STATUS.  0 ok; 1 unreachable; 2 the start or goal cell is outside the grid, or the start heading is outside 0 .. 7.
// REFUSED before launch, nothing is clamped: a cost outside 0 .. 255, L not 1 or 8, 16 * rows * cols * (1 + turn_cost +
//   reverse_cost + cusp_cost) >= 2^21 (the bound under which the float64 key orders pairs exactly, on the largest count a
//   path over 16 * rows * cols states can reach), a short or misaligned workspace, null required pointers.
#include "common.h"
#include "pair_cost.h"

namespace nfopp {

constexpr int LG_THREADS = 512;
constexpr int LG_HEADINGS = 8;
constexpr int LG_STATES = 16;           // layers of a field: gear * 8 + heading
constexpr int LG_BATCH = 2;             // cells of a line a thread has in flight: their 7 reads each are issued before any is used
constexpr int LG_LDS_WORDS = 36864;     // packed 16-layer field in LDS up to 144 KiB
constexpr long long LG_MAX_COUNT = 1LL << 21;

__constant__ int LG_DR[LG_HEADINGS] = {0, 1, 1, 1, 0, -1, -1, -1};
__constant__ int LG_DC[LG_HEADINGS] = {1, 1, 0, -1, -1, -1, 0, 1};

struct GearFieldArgs {
  const unsigned char* occ;   // [L, rows, cols]
  const int* goals;           // [G, 3] (row, col, heading or -1)
  int layers, rows, cols, stride, turn_cost, reverse_cost, cusp_cost;
  long long padded;           // cells of one padded layer
  int* out;                   // [G, 2, 8, rows, cols, 2]
  void* work;                 // wide path: G padded 16-layer fields of uint64
};

// the smaller of (best, w) by the pair order; the candidate's key is formed from its own pair, as the stored value's is, so
// equal pairs have equal keys and the first stays
template <class T>
__device__ __forceinline__ void gear_take(T w, T& best, double& best_k) {
  const double k = pair_key(w);
  if (k < best_k) { best_k = k; best = w; }
}

// One workgroup per goal state.  F holds 16 padded layers (gear * 8 + heading) of (rows + 2) x stride cells with a blocked
// border all round, so every successor of a cell of the image is read without a bounds test.  A thread takes a LINE of one
// heading h, as in lattice_search.hip: the cells along dir(h).  It owns both gears of the line's cells and walks it twice
// a sweep.  Pass 1 goes against the heading from the far end and carries d(0, h, .) of the cell ahead in a register, so a
// straight forward run of any length settles in one sweep; pass 2 goes with the heading from the near end and carries
// d(1, h, .) of the cell behind, so a straight reverse run does.  At a cell both passes form
//   FW = min over h' of d(0, h', c + dir(h')) + length(h') + turn,   RV = min over h' of d(1, h', c - dir(h)) + length(h) + turn
//        + reverse_cost
// and lower d(0, h, c) to min(FW, RV + cusp) and d(1, h, c) to min(FW + cusp, RV): seven reads and the carried value for
// two states, the reads of LG_BATCH cells issued before the arithmetic of the first.  The turning reverse successors sit
// at the neighbouring cell c - dir(h), not in place.  Lanes hold neighbouring lines: their reads are consecutive cells or
// `stride` apart, and stride is odd, so a half-wave of ds_read_b32 never meets twice on one of the 32 banks.  Sweeps are
// in place and unsynchronised inside: every state has one owner, every value ever stored is the cost of a real path and
// values only fall, so a sweep in which no state changed (workgroup-wide OR) is the fixed point.  After k sweeps the k
// nearest states are final, so at most 16 * rows * cols sweeps are made.
template <class T>
__device__ __forceinline__ void gear_field_body(const GearFieldArgs& a, T* F, int g) {
  using P = Packed<T>;
  const int rows = a.rows, cols = a.cols, stride = a.stride;
  const long long padded = a.padded, cells = (long long)rows * cols;
  const int gr = a.goals[3 * g], gc = a.goals[3 * g + 1], gh = a.goals[3 * g + 2];
  const bool goal_ok = gr >= 0 && gr < rows && gc >= 0 && gc < cols && gh >= -1 && gh < LG_HEADINGS;
  int2* out = reinterpret_cast<int2*>(a.out) + (long long)g * LG_STATES * cells;
  if (!goal_ok) {   // uniform over the workgroup
    for (long long k = threadIdx.x; k < LG_STATES * cells; k += LG_THREADS) out[k] = make_int2(-1, -1);
    return;
  }
  for (int h = 0; h < LG_HEADINGS; ++h) {
    const unsigned char* occ = a.occ + (long long)(h % a.layers) * cells;
    for (long long j = threadIdx.x; j < padded; j += LG_THREADS) {
      const int r = (int)(j / stride) - 1, c = (int)(j % stride) - 1;
      T v = P::WALL;
      if (r >= 0 && r < rows && c >= 0 && c < cols) {
        if (occ[(long long)r * cols + c] == 0) v = P::UNREACHED;
        if (r == gr && c == gc && (gh < 0 || gh == h)) v = 0;   // goal states are forced free, at both gears
      }
      F[h * padded + j] = v;
      F[(LG_HEADINGS + h) * padded + j] = v;
    }
  }
  if (sizeof(T) == 8) __threadfence();
  __syncthreads();
  const long long max_sweeps = LG_STATES * cells + 1;
  const T turn = (T)a.turn_cost * P::STRAIGHT;
  const T rev = (T)a.reverse_cost * P::STRAIGHT;
  const T cusp = (T)a.cusp_cost * P::STRAIGHT;
  const int n_diag = rows + cols - 1;
  const int n_lines = 2 * rows + 2 * cols + 4 * n_diag;
  for (long long sweep = 0; sweep < max_sweeps; ++sweep) {
    int changed = 0;
    for (int q = threadIdx.x; q < n_lines; q += LG_THREADS) {
      // line q -> (heading, line of that heading): rows for h = 0, 4; columns for h = 2, 6; diagonals for odd h
      int h = 0, i = q;
      for (; h < LG_HEADINGS - 1; ++h) {
        const int n = (h & 1) ? n_diag : ((h & 2) ? cols : rows);
        if (i < n) break;
        i -= n;
      }
      const int dr = LG_DR[h], dc = LG_DC[h];
      // (r, c): the far end of the line, the cell whose straight forward successor is outside the image; len: its cells
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
      T* own1 = F + (LG_HEADINGS + h) * padded;
      const T* fl_p = F + hl * padded + (LG_DR[hl] * stride + LG_DC[hl]);   // forward turn successors: gear 0, c + dir(h')
      const T* fr_p = F + hr * padded + (LG_DR[hr] * stride + LG_DC[hr]);
      const T* bl_p = F + (LG_HEADINGS + hl) * padded - step;               // reverse turn successors: gear 1, c - dir(h)
      const T* br_p = F + (LG_HEADINGS + hr) * padded - step;
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
  for (int l = 0; l < LG_STATES; ++l)
    for (long long k = threadIdx.x; k < cells; k += LG_THREADS) {
      const int r = (int)(k / cols), c = (int)(k % cols);
      const T v = F[l * padded + (long long)(r + 1) * stride + c + 1];
      out[l * cells + k] = v >= P::WALL ? make_int2(-1, -1) : make_int2(P::a(v), P::b(v));
    }
}

__global__ __launch_bounds__(LG_THREADS) void gear_field_lds_kernel(const GearFieldArgs a) {
  extern __shared__ uint32_t lg_lds[];
  gear_field_body<uint32_t>(a, lg_lds, blockIdx.x);
}

__global__ __launch_bounds__(LG_THREADS) void gear_field_wide_kernel(const GearFieldArgs a) {
  gear_field_body<uint64_t>(a, reinterpret_cast<uint64_t*>(a.work) + (long long)blockIdx.x * LG_STATES * a.padded, blockIdx.x);
}

// ---- descent through the field, one problem per thread ------------------------------------------------------------------
struct GearTraceArgs {
  const int* fields;         // [n_fields, 2, 8, rows, cols, 2]: fields field_first .. field_first + n_fields - 1 of n_total
  const int* start_states;   // [B, 3] (row, col, heading)
  const int* goal_states;    // [B, 3] (row, col, heading or -1)
  const int* field_index;    // [B]
  int rows, cols, turn_cost, reverse_cost, cusp_cost, max_len;
  long long batch, field_first, n_fields, n_total;
  int* cells;                // [B, max_len, 2]
  int* headings;             // [B, max_len]
  int* gears;                // [B, max_len]
  int* count; int* status; int* cost;
};

// Successor i = 0 .. 5 of (r, c, h) in the order of the rule: forward h, h + 1, h - 1, then reverse h, h + 1, h - 1.
// -> false: its cell is outside the grid.  (*ma, *mb): the move's cost without the cusp term.
__device__ __forceinline__ bool gear_successor(int r, int c, int h, int i, int rows, int cols, int tc, int rc, int* nr, int* nc,
                                               int* nh, int* ns, int* ma, int* mb) {
  const int t = i % 3;
  const int hn = t == 0 ? h : (t == 1 ? (h + 1) & 7 : (h + 7) & 7);
  const int s = i / 3;
  const int along = s ? h : hn;   // a reverse move backs along the heading before it
  *nr = s ? r - LG_DR[h] : r + LG_DR[hn];
  *nc = s ? c - LG_DC[h] : c + LG_DC[hn];
  *nh = hn; *ns = s;
  *ma = ((along & 1) ? 0 : 1) + (hn != h ? tc : 0) + (s ? rc : 0);
  *mb = along & 1;
  return *nr >= 0 && *nr < rows && *nc >= 0 && *nc < cols;
}

__global__ __launch_bounds__(256) void gear_trace_kernel(const GearTraceArgs a) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.batch) return;
  const int rows = a.rows, cols = a.cols, tc = a.turn_cost, rc = a.reverse_cost, cc = a.cusp_cost;
  const long long cells_n = (long long)rows * cols;
  int r = a.start_states[3 * p], c = a.start_states[3 * p + 1], h = a.start_states[3 * p + 2];
  const int gr = a.goal_states[3 * p], gc = a.goal_states[3 * p + 1];
  const long long fi = a.field_index[p];
  int status = 0, count = 0, ca = -1, cb = -1;
  if (r < 0 || r >= rows || c < 0 || c >= cols || h < 0 || h >= LG_HEADINGS || gr < 0 || gr >= rows || gc < 0 || gc >= cols ||
      fi < 0 || fi >= a.n_total) {
    status = 2;
  } else if (fi < a.field_first || fi >= a.field_first + a.n_fields) {
    return;   // the problem's field is not among the ones of this call: nothing of it is touched
  } else {
    const int2* f = reinterpret_cast<const int2*>(a.fields) + (fi - a.field_first) * LG_STATES * cells_n;
    int2* cells = a.max_len > 0 ? reinterpret_cast<int2*>(a.cells) + p * a.max_len : nullptr;
    int* heads = a.max_len > 0 ? a.headings + p * a.max_len : nullptr;
    int* gears = a.max_len > 0 ? a.gears + p * a.max_len : nullptr;
    int2 d = f[h * cells_n + (long long)r * cols + c];   // goal states hold (0, 0) at both gears, and only they do
    int len = 0, s = 0;
    if (d.x == 0 && d.y == 0) {
      if (cells) { cells[0] = make_int2(r, c); heads[0] = h; gears[0] = 0; }
      len = 1; ca = cb = 0;
    } else {
      double best = INFINITY;
      int bi = -1;
      for (int i = 0; i < 6; ++i) {
        int nr, nc, nh, ns, ma, mb;
        if (!gear_successor(r, c, h, i, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
        const int2 dn = f[(ns * LG_HEADINGS + nh) * cells_n + (long long)nr * cols + nc];
        if (dn.x < 0) continue;
        const double k = pair_key(dn.x + ma, dn.y + mb);   // equal pairs give equal keys: the first in order stays
        if (k < best) { best = k; bi = i; ca = dn.x + ma; cb = dn.y + mb; }
      }
      if (bi < 0) status = 1;
      else {
        int nr, nc, nh, ns, ma, mb;
        gear_successor(r, c, h, bi, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb);
        if (cells) { cells[0] = make_int2(r, c); heads[0] = h; gears[0] = ns; }
        len = 1;
        r = nr; c = nc; h = nh; s = ns;
        d = f[(s * LG_HEADINGS + h) * cells_n + (long long)r * cols + c];
        // every move lowers a + b by at least one, so the walk ends; the bound keeps a field that is no fixed point finite
        const long long max_steps = LG_STATES * cells_n;
        for (long long step = 0;; ++step) {
          if (cells && len < a.max_len) { cells[len] = make_int2(r, c); heads[len] = h; gears[len] = s; }
          ++len;
          if ((d.x == 0 && d.y == 0) || step >= max_steps) break;
          int pick = -1;
          int2 dn = d;
          for (int i = 0; i < 6 && pick < 0; ++i) {
            if (!gear_successor(r, c, h, i, rows, cols, tc, rc, &nr, &nc, &nh, &ns, &ma, &mb)) continue;
            dn = f[(ns * LG_HEADINGS + nh) * cells_n + (long long)nr * cols + nc];
            if (dn.x >= 0 && dn.x + ma + (ns != s ? cc : 0) == d.x && dn.y + mb == d.y) pick = i;
          }
          if (pick < 0) break;   // cannot happen on a fixed-point field
          r = nr; c = nc; h = nh; s = ns;
          d = dn;
        }
        if (d.x != 0 || d.y != 0) status = 1;   // a caller's field that is no fixed point: the walk did not reach the goal
      }
    }
    if (status == 0) count = len;
    else ca = cb = -1;
  }
  a.count[p] = count;
  a.status[p] = status;
  if (a.cost) { a.cost[2 * p] = ca; a.cost[2 * p + 1] = cb; }
}

// -> false: refused.  *lds: the packed form in LDS applies.
static bool gear_shape(int rows, int cols, int turn_cost, int reverse_cost, int cusp_cost, int* stride, long long* padded, bool* lds) {
  if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768 || turn_cost < 0 || turn_cost > 255 || reverse_cost < 0 ||
      reverse_cost > 255 || cusp_cost < 0 || cusp_cost > 255) return false;
  const long long counts = (long long)LG_STATES * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost);
  if (counts >= LG_MAX_COUNT) return false;
  *stride = (cols + 2) | 1;   // odd: lines a row apart fall on different LDS banks
  *padded = (long long)(rows + 2) * *stride;
  *lds = LG_STATES * *padded <= LG_LDS_WORDS && counts <= 65535;   // no 16-bit count can wrap
  return true;
}

}  // namespace nfopp

using namespace nfopp;

#define LG_REQUIRE_COSTS()                                                                                     \
  NFOPP_REQUIRE(turn_cost >= 0 && turn_cost <= 255, "turn_cost must be 0..255, not %d", turn_cost);             \
  NFOPP_REQUIRE(reverse_cost >= 0 && reverse_cost <= 255, "reverse_cost must be 0..255, not %d", reverse_cost); \
  NFOPP_REQUIRE(cusp_cost >= 0 && cusp_cost <= 255, "cusp_cost must be 0..255, not %d", cusp_cost)

extern "C" size_t nfopp_lattice_gear_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost,
                                                            int32_t cusp_cost, int64_t n_goals) {
  int stride;
  long long padded;
  bool lds;
  if (n_goals < 1 || !gear_shape(rows, cols, turn_cost, reverse_cost, cusp_cost, &stride, &padded, &lds) || lds) return 0;
  return (size_t)padded * LG_STATES * 8 * (size_t)n_goals;
}

extern "C" int nfopp_lattice_gear_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                                  const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost,
                                                  int32_t reverse_cost, int32_t cusp_cost, int32_t* fields_dev,
                                                  void* workspace_dev, size_t workspace_bytes, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768, "grid must be 1..32768 cells a side");
  NFOPP_REQUIRE(n_layers == 1 || n_layers == 8, "occupancy must have 1 or 8 layers, not %d", n_layers);
  LG_REQUIRE_COSTS();
  GearFieldArgs a;
  bool lds;
  NFOPP_REQUIRE(gear_shape(rows, cols, turn_cost, reverse_cost, cusp_cost, &a.stride, &a.padded, &lds),
                "16 * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost) reaches 2^21: path counts could leave the "
                "exactly ordered range");
  NFOPP_REQUIRE(n_goals >= 0 && n_goals <= 0x7fffffffLL, "bad goal count");
  if (n_goals == 0) return NFOPP_OK;
  NFOPP_REQUIRE(layers_dev && goal_states_dev && fields_dev, "null device pointer");
  a.occ = layers_dev; a.goals = goal_states_dev; a.layers = n_layers; a.rows = rows; a.cols = cols; a.turn_cost = turn_cost;
  a.reverse_cost = reverse_cost; a.cusp_cost = cusp_cost; a.out = fields_dev; a.work = nullptr;
  if (lds) {
    static bool attr_set[MAX_DEVICES] = {};
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(gear_field_lds_kernel), (size_t)LG_LDS_WORDS * 4, attr_set);
    if (rc != NFOPP_OK) return rc;
    hipLaunchKernelGGL(gear_field_lds_kernel, dim3((unsigned)n_goals), dim3(LG_THREADS), (size_t)a.padded * LG_STATES * 4,
                       (hipStream_t)stream, a);
  } else {
    const size_t need = (size_t)a.padded * LG_STATES * 8 * (size_t)n_goals;
    NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small: nfopp_lattice_gear_fields_workspace_bytes gives %zu", need);
    NFOPP_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace must be 8-byte aligned");
    a.work = workspace_dev;
    hipLaunchKernelGGL(gear_field_wide_kernel, dim3((unsigned)n_goals), dim3(LG_THREADS), 0, (hipStream_t)stream, a);
  }
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_lattice_gear_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                                              int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost,
                                              int32_t cusp_cost, const int32_t* start_states_dev, const int32_t* goal_states_dev,
                                              const int32_t* field_index_dev, int64_t batch, int32_t max_len, int32_t* cells_dev,
                                              int32_t* headings_dev, int32_t* gears_dev, int32_t* count_dev, int32_t* status_dev,
                                              int32_t* cost_dev, void* stream) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768 && max_len >= 0, "bad sizes");
  LG_REQUIRE_COSTS();
  NFOPP_REQUIRE((long long)LG_STATES * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost) < LG_MAX_COUNT,
                "grid and costs beyond the limit of nfopp_lattice_gear_distance_fields");
  NFOPP_REQUIRE(field_first >= 0 && n_fields >= 0 && n_total >= 0 && field_first + n_fields <= n_total, "bad field range");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL, "bad batch");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(start_states_dev && goal_states_dev && field_index_dev && count_dev && status_dev, "null device pointer");
  NFOPP_REQUIRE((fields_dev || n_fields == 0) && ((cells_dev && headings_dev && gears_dev) || max_len == 0), "null device pointer");
  GearTraceArgs a;
  a.fields = fields_dev; a.start_states = start_states_dev; a.goal_states = goal_states_dev; a.field_index = field_index_dev;
  a.rows = rows; a.cols = cols; a.turn_cost = turn_cost; a.reverse_cost = reverse_cost; a.cusp_cost = cusp_cost;
  a.max_len = max_len; a.batch = batch; a.field_first = field_first; a.n_fields = n_fields; a.n_total = n_total;
  a.cells = cells_dev; a.headings = headings_dev; a.gears = gears_dev; a.count = count_dev; a.status = status_dev; a.cost = cost_dev;
  hipLaunchKernelGGL(gear_trace_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
