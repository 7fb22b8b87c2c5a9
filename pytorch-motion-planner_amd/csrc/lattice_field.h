// What the lattice searches share: lattice_search.hip over (cell, heading) states, lattice_gears.hip over (cell, heading,
// gear) states.  grid_search.hip takes the fill and the store of a padded layer for its one-layer field.
// OWNED HERE, once: the direction table; the map from a line number to a line; the padded field frame (fill, sentinel field,
// store); the shape predicate, the workspace size and the field entry with its LDS-or-workspace launch; the cost-range
// refusal; of the trace the successor order, the problem prologue, the record of a state, the epilogue and the launch.
// STAYS PER SEARCH, written out in each file: the relaxation of a line (3 reads and one walk, LS_BATCH = 4, against 7 reads
// and two walks, LG_BATCH = 2) and the trace's start rule and walk.  The rules differ: forward only takes the minimum over
// its successors ONLY at a blocked start (elsewhere the start's own cost leads the descent) and reports `count` on a
// caller's field that is no fixed point; with gears the first move is ALWAYS the minimum over the six successors without
// the cusp term, and such a field gives status 1.  A further variant is a new relaxation and start rule on these parts,
// not a mode parameter.  The generated code follows the spelling closely (profiles/lattice_field.txt), and a helper that moved
// a kernel's time beyond the parent's run-to-run spread is not used there: lattice_gears.hip keeps its own text of the goal
// decode, the fill and the line map, the same as lattice_goal, lattice_fill_layer and lattice_line below.
// DIRECTIONS.  Heading h in 0 .. 7 stands for the angle h * pi / 4; dir(h) as (d row, d col), row = y and col = x:
//   h      0       1       2       3       4        5        6       7
//   dir  (0,+1)  (+1,+1)  (+1,0)  (+1,-1)  (0,-1)  (-1,-1)  (-1,0)  (-1,+1)
// FIELD FRAME.  One workgroup per goal state relaxes a field of padded layers: (rows + 2) x stride cells each, a blocked
//   border all round, so the successors of a cell of the image are read without a bounds test.  A thread takes LINES: the
//   cells of one heading's layer along dir(h), a row for h = 0, 4, a column for h = 2, 6, a diagonal for odd h.  Lanes hold
//   neighbouring lines: their reads are consecutive cells or `stride` apart, and stride is odd, so a half-wave of
//   ds_read_b32 never meets twice on one of the 32 banks.  Sweeps are in place and unsynchronised inside: every state has
//   one owner, every value stored is the cost of a real path and values only fall, so a sweep in which no state changed
//   (workgroup-wide OR) is the fixed point; after k sweeps the k nearest states are final.
#pragma once
#include <initializer_list>
#include <utility>

#include "common.h"
#include "pair_cost.h"

namespace nfopp {

constexpr int LATTICE_THREADS = 512;
constexpr int LATTICE_HEADINGS = 8;
constexpr int LATTICE_LDS_WORDS = 36864;            // packed field of all state layers in LDS up to 144 KiB
constexpr long long LATTICE_MAX_COUNT = 1LL << 21;  // the bound under which the float64 key orders pairs exactly

// `inline`: one definition however many translation units include this header.  Not `static`: with internal linkage the
// compiler reads the table at compile time and rebuilds the field kernels around its values (profiles/lattice_field.txt).
inline __constant__ int LATTICE_DR[LATTICE_HEADINGS] = {0, 1, 1, 1, 0, -1, -1, -1};
inline __constant__ int LATTICE_DC[LATTICE_HEADINGS] = {1, 1, 0, -1, -1, -1, 0, 1};

// the arguments of a field kernel and of a trace kernel; the forward-only search has reverse_cost = cusp_cost = 0, no gears
struct LatticeFieldArgs {
  const unsigned char* occ;   // [L, rows, cols]
  const int* goals;           // [G, 3] (row, col, heading or -1)
  int layers, rows, cols, stride, turn_cost, reverse_cost, cusp_cost;
  long long padded;           // cells of one padded layer
  int* out;                   // [G, 8, rows, cols, 2], with gears [G, 2, 8, rows, cols, 2]
  void* work;                 // wide path: G padded fields of uint64
};
struct LatticeTraceArgs {
  const int* fields;         // [n_fields] fields as LatticeFieldArgs::out: fields field_first .. field_first + n_fields - 1 of n_total
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

__device__ __forceinline__ int lattice_n_lines(int rows, int cols) { return 2 * rows + 2 * cols + 4 * (rows + cols - 1); }

struct LatticeLine {
  int h, len, step;   // heading; cells; one cell along the heading, as an index step in a padded layer
  long long far;      // index in the padded layer of the far end: the cell whose straight successor is outside the image
};

// line q of lattice_n_lines(rows, cols), numbered heading by heading
__device__ __forceinline__ LatticeLine lattice_line(int q, int rows, int cols, int stride) {
  const int n_diag = rows + cols - 1;
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
  return {h, len, dr * stride + dc, (long long)(r + 1) * stride + c + 1};
}

// Goal state g of goals [G, 3] (row, col, heading or -1).  -> false: its cell is outside the grid or its heading outside
// -1 .. 7, and out [n] has been filled with the sentinel (-1, -1), the whole field of such a goal.
template <int THREADS>
__device__ __forceinline__ bool lattice_goal(const int* goals, int g, int rows, int cols, int* gr, int* gc, int* gh, int2* out,
                                             long long n) {
  *gr = goals[3 * g]; *gc = goals[3 * g + 1]; *gh = goals[3 * g + 2];
  if (*gr >= 0 && *gr < rows && *gc >= 0 && *gc < cols && *gh >= -1 && *gh < LATTICE_HEADINGS) return true;
  for (long long k = threadIdx.x; k < n; k += THREADS) out[k] = make_int2(-1, -1);
  return false;
}

// Fills the padded layer F from the occupancy image occ [rows, cols]: border and blocked cells WALL, free cells UNREACHED,
// and on a goal layer the goal cell (gr, gc) 0 -- goal states are forced free.  With COPIES = 2 every value also goes to
// the layer `twin` cells behind F (the other gear of the same heading).
template <class T, int THREADS, int COPIES = 1>
__device__ __forceinline__ void lattice_fill_layer(T* F, const unsigned char* occ, int rows, int cols, int stride, long long padded,
                                                   int gr, int gc, bool goal_layer, long long twin = 0) {
  for (long long j = threadIdx.x; j < padded; j += THREADS) {
    const int r = (int)(j / stride) - 1, c = (int)(j % stride) - 1;
    T v = Packed<T>::WALL;
    if (r >= 0 && r < rows && c >= 0 && c < cols) {
      if (occ[(long long)r * cols + c] == 0) v = Packed<T>::UNREACHED;
      if (r == gr && c == gc && goal_layer) v = 0;
    }
    F[j] = v;
    if (COPIES == 2) F[twin + j] = v;
  }
}

// the interior of the padded layer that starts at F[f0] -> out[o0 ..], `cells` = rows * cols pairs (a, b), (-1, -1) for what
// has no cost.  Offsets, not advanced pointers: that is the spelling under which the gear kernels keep their instructions.
template <class T, int THREADS>
__device__ __forceinline__ void lattice_store_layer(const T* F, long long f0, int2* out, long long o0, long long cells, int cols,
                                                    int stride) {
  using P = Packed<T>;
  for (long long k = threadIdx.x; k < cells; k += THREADS) {
    const int r = (int)(k / cols), c = (int)(k % cols);
    const T v = F[f0 + (long long)(r + 1) * stride + c + 1];
    out[o0 + k] = v >= P::WALL ? make_int2(-1, -1) : make_int2(P::a(v), P::b(v));
  }
}

// ---- the trace: one problem per thread -------------------------------------------------------------------------------------
// Successor i = 0 .. 5 of (r, c, h) in the order of the rule: forward h, h + 1, h - 1, then reverse h, h + 1, h - 1; the
// forward-only search stops at i < 3.  A forward move goes along the heading AFTER it, a reverse move backs along the one
// BEFORE it.  -> false: its cell is outside the grid.  (*ma, *mb): the move's cost without the cusp term.
__device__ __forceinline__ bool lattice_successor(int r, int c, int h, int i, int rows, int cols, int tc, int rc, int* nr, int* nc,
                                                  int* nh, int* ns, int* ma, int* mb) {
  const int t = i % 3;
  const int hn = t == 0 ? h : (t == 1 ? (h + 1) & 7 : (h + 7) & 7);
  const int s = i / 3;
  const int along = s ? h : hn;
  *nr = s ? r - LATTICE_DR[h] : r + LATTICE_DR[hn];
  *nc = s ? c - LATTICE_DC[h] : c + LATTICE_DC[hn];
  *nh = hn; *ns = s;
  *ma = ((along & 1) ? 0 : 1) + (hn != h ? tc : 0) + (s ? rc : 0);
  *mb = along & 1;
  return *nr >= 0 && *nr < rows && *nc >= 0 && *nc < cols;
}

// Problem p -> 2: its status (the start or goal cell is outside the grid, or the start heading
// outside 0 .. 7); -1: its field is not among the ones of this call and nothing of it may be touched; 0: (*r, *c, *h) is its
// start state and *f its field of n_state_layers layers.
__device__ __forceinline__ int lattice_trace_begin(const LatticeTraceArgs& a, long long p, int n_state_layers, int* r, int* c, int* h,
                                                   const int2** f) {
  const int rows = a.rows, cols = a.cols;
  *r = a.start_states[3 * p]; *c = a.start_states[3 * p + 1]; *h = a.start_states[3 * p + 2];
  const int gr = a.goal_states[3 * p], gc = a.goal_states[3 * p + 1];
  const long long fi = a.field_index[p];
  if (*r < 0 || *r >= rows || *c < 0 || *c >= cols || *h < 0 || *h >= LATTICE_HEADINGS || gr < 0 || gr >= rows || gc < 0 ||
      gc >= cols || fi < 0 || fi >= a.n_total) return 2;
  if (fi < a.field_first || fi >= a.field_first + a.n_fields) return -1;
  *f = reinterpret_cast<const int2*>(a.fields) + (fi - a.field_first) * n_state_layers * ((long long)rows * cols);
  return 0;
}

__device__ __forceinline__ void lattice_record(int2* cells, int* heads, int k, int r, int c, int h) {
  cells[k] = make_int2(r, c);
  heads[k] = h;
}

// what a problem reports: no states and the cost (-1, -1) unless its status is 0
__device__ __forceinline__ void lattice_trace_end(int* count, int* status, int* cost, long long p, int len, int st, int ca, int cb) {
  count[p] = st == 0 ? len : 0;
  status[p] = st;
  if (cost) { cost[2 * p] = st == 0 ? ca : -1; cost[2 * p + 1] = st == 0 ? cb : -1; }
}

// ---- host: shape, refusals, launch -----------------------------------------------------------------------------------------
// the one range of a cost and the one text of its refusal
constexpr bool lattice_cost_ok(int cost) { return cost >= 0 && cost <= 255; }
#define LATTICE_REQUIRE_COST_NAMED(name, cost) NFOPP_REQUIRE(lattice_cost_ok(cost), "%s must be 0..255, not %d", name, cost)
#define LATTICE_REQUIRE_COST(cost) LATTICE_REQUIRE_COST_NAMED(#cost, cost)
// 1 + the costs of a search: the largest count one move adds.  -> 0, which lattice_shape refuses, where one is outside 0 .. 255.
static long long lattice_cost_sum(int turn_cost, int reverse_cost = 0, int cusp_cost = 0) {
  const bool ok = lattice_cost_ok(turn_cost) && lattice_cost_ok(reverse_cost) && lattice_cost_ok(cusp_cost);
  return ok ? 1 + turn_cost + reverse_cost + cusp_cost : 0;
}

// -> false: refused.  *lds: the packed form in LDS applies.
static bool lattice_shape(int rows, int cols, int n_state_layers, long long cost_sum, int* stride, long long* padded, bool* lds) {
  if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768 || cost_sum < 1) return false;
  const long long counts = (long long)n_state_layers * rows * cols * cost_sum;
  if (counts >= LATTICE_MAX_COUNT) return false;
  *stride = (cols + 2) | 1;   // odd: lines a row apart fall on different LDS banks
  *padded = (long long)(rows + 2) * *stride;
  *lds = n_state_layers * *padded <= LATTICE_LDS_WORDS && counts <= 65535;   // no 16-bit count can wrap
  return true;
}

// bytes of the wide fields of n_goals goals: 0 where the shape is refused or relaxes in LDS
static size_t lattice_workspace_bytes(int rows, int cols, int n_state_layers, long long cost_sum, long long n_goals) {
  int stride;
  long long padded;
  bool lds;
  if (n_goals < 1 || !lattice_shape(rows, cols, n_state_layers, cost_sum, &stride, &padded, &lds) || lds) return 0;
  return (size_t)padded * n_state_layers * 8 * (size_t)n_goals;
}

// A field entry from its first check to its launch: `costs` is (name, value) of the search's costs in the order turn,
// reverse, cusp; `beyond` and `too_small` (with %zu for the size) are the entry's own texts.  One workgroup per goal:
// LDS_KERNEL on the packed field where it fits, else WIDE_KERNEL on the caller's workspace.
template <auto LDS_KERNEL, auto WIDE_KERNEL>
int lattice_fields_entry(const uint8_t* layers_dev, int n_layers, int rows, int cols, const int32_t* goal_states_dev, long long n_goals,
                         std::initializer_list<std::pair<const char*, int>> costs, int32_t* fields_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream, int n_state_layers, const char* beyond, const char* too_small) {
  NFOPP_REQUIRE(rows >= 1 && cols >= 1 && rows <= 32768 && cols <= 32768, "grid must be 1..32768 cells a side");
  NFOPP_REQUIRE(n_layers == 1 || n_layers == 8, "occupancy must have 1 or 8 layers, not %d", n_layers);
  int cost[3] = {0, 0, 0}, k = 0;
  for (const auto& c : costs) {
    LATTICE_REQUIRE_COST_NAMED(c.first, c.second);
    cost[k++] = c.second;
  }
  LatticeFieldArgs a = {layers_dev, goal_states_dev, n_layers, rows, cols, 0, cost[0], cost[1], cost[2], 0, fields_dev, nullptr};
  bool lds;
  const long long cost_sum = lattice_cost_sum(cost[0], cost[1], cost[2]);
  NFOPP_REQUIRE(lattice_shape(rows, cols, n_state_layers, cost_sum, &a.stride, &a.padded, &lds), "%s", beyond);
  NFOPP_REQUIRE(n_goals >= 0 && n_goals <= 0x7fffffffLL, "bad goal count");
  if (n_goals == 0) return NFOPP_OK;
  NFOPP_REQUIRE(layers_dev && goal_states_dev && fields_dev, "null device pointer");
  if (lds) {
    static bool attr_set[MAX_DEVICES] = {};   // one per LDS_KERNEL
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(LDS_KERNEL), (size_t)LATTICE_LDS_WORDS * 4, attr_set);
    if (rc != NFOPP_OK) return rc;
    hipLaunchKernelGGL(LDS_KERNEL, dim3((unsigned)n_goals), dim3(LATTICE_THREADS), (size_t)a.padded * n_state_layers * 4,
                       (hipStream_t)stream, a);
  } else {
    const size_t need = (size_t)a.padded * n_state_layers * 8 * (size_t)n_goals;
    NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, too_small, need);
    NFOPP_REQUIRE(((uintptr_t)workspace_dev & 7) == 0, "workspace must be 8-byte aligned");
    a.work = workspace_dev;
    hipLaunchKernelGGL(WIDE_KERNEL, dim3((unsigned)n_goals), dim3(LATTICE_THREADS), 0, (hipStream_t)stream, a);
  }
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// the tail of a trace entry, behind its size, cost and count checks; paths_ok: every per-state output has a pointer
template <auto KERNEL>
int lattice_trace_launch(const LatticeTraceArgs& a, bool paths_ok, void* stream) {
  NFOPP_REQUIRE(a.field_first >= 0 && a.n_fields >= 0 && a.n_total >= 0 && a.field_first + a.n_fields <= a.n_total, "bad field range");
  NFOPP_REQUIRE(a.batch >= 0 && a.batch <= 0x7fffffffLL, "bad batch");
  if (a.batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(a.start_states && a.goal_states && a.field_index && a.count && a.status, "null device pointer");
  NFOPP_REQUIRE((a.fields || a.n_fields == 0) && (paths_ok || a.max_len == 0), "null device pointer");
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

}  // namespace nfopp
