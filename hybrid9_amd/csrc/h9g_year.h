// h9g_year.h -- the year kernels and their launch: the kernels' arguments,
// the table of launch shapes (H9G_YEAR_SHAPES: one row per kernel, from which
// the kernel definitions, the launch's cases and the reported names are
// made), the kernel kinds, the geometry dispatch and launch_shape.  Included
// by h9g_plain.hip, which instantiates the plain kernels, by h9g_mon.hip,
// which instantiates the monthly ones, by h9g_et.hip, which instantiates
// the evapotranspiration (ET) ones, and by h9g_day.hip, which instantiates the
// day-record ones, so that the four compile side by side
// (hybrid9_amd/build.py), beside h9g_cols.hip with the other
// geometry-templated kernels; tools/isa_unit.hip instantiates single kernels
// for the ISA study.  At its end: the kernel units' launchers, which is all
// the host runtime's units (h9g_ctx.h) see of them.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/h9g.h"
#include "h9_math.h"
#include "h9g_geo.h"
#include "h9g_step.h"
#include "h9g_pair.h"
#include "h9g_rows.h"

using namespace h9k;

#define H9G_YBLOCK 64   // solo kernel: one wave per block (LDS cell stores)
// pair kernel: 22 columns (44 lanes) per wave, 4 waves per workgroup; the
// 0.5 deg grid is 767 workgroups = 3 waves on each of the 1,024 SIMDs
#define H9G_PCPW 22
#define H9G_PLANES (2 * H9G_PCPW)
#define H9G_PWAVES 4
#define H9G_PCPW11 11   // the 11-column kernel

// ---------------------------------------------------------------------------
// kernel arguments
// ---------------------------------------------------------------------------
struct KArgs {
  int ncell;       // row stride of every per-cell array
  int c0, cend;    // cells [c0, cend) of this launch
  int nt;          // days in the year
  int nisurf;
  int grow_on;
  size_t fvar;     // forcing variable stride (floats) = max_days * ncell
  const float *__restrict__ par;   // parameter rows x ncell (h9g_rows.h)
  float *__restrict__ st;          // state rows x ncell
  const float *__restrict__ forc;  // 7 x max_days x ncell (slot base)
  float *__restrict__ annual;      // annual rows x ncell
  int *__restrict__ err;           // STOP record rows x ncell
  int *__restrict__ err_flag;
  unsigned *__restrict__ stamps;   // H9G_STAMPS builds: 8 phase cycle sums per wave
  float *__restrict__ sv;          // pair kernel: day snapshot, PairStore::GBLOCK bytes per workgroup
  const int *__restrict__ perm;    // lane slot -> cell (h9g_sort_kernel), or null: identity
  int sorted_io;                   // 1: forc and annual are in slot order (h9g_perm_forcing_kernel; round 4)
  int *__restrict__ hist;          // per cell: substeps of the year with the water table below the column
  unsigned *__restrict__ pace;     // pair kernel, Pacer mode 2: H9G_PACE_ROWS x 16 progress words
  unsigned epoch;                  // Pacer mode 2: launch tag
  int prio_mode;                   // Pacer mode: 0 none, 1 rotate, 2 pace
  // A second group of cells in the same launch (pair kernels; the cell-order
  // mode's re-runs of one decade riding in the next decade's year launches,
  // h9g_run_ordered).  Slots [c0, bend) are the first group; the waves from
  // slot `split` (a multiple of the wave's column count, >= bend) to cend
  // the second, with their own state and error rows, year length and no
  // sort history.  split == cend: no second group.
  int bend, split, nt2;
  float *__restrict__ st2;
  int *__restrict__ err2;
  size_t iostride;                 // row stride of forc and annual when sorted_io (slots)
  int raw;                         // 1: the annual rows are the running sums, undivided (the cell
                                   // order's day-1 probe, h9g_probe_cmp_kernel)
};

// XCD-aware workgroup order.  MI355X deals the workgroups of a launch
// round-robin to its 8 XCDs (workgroup b -> XCD b % 8), each with its own L2.
// Workgroup b works on the cells of virtual workgroup xcd_vwg(b), which makes
// each XCD's workgroups one contiguous range of cells: the forcing, annual
// sums and state lines an XCD touches are its own (no line fetched by two
// XCDs), and the per-year cell sort (h9g_sort_kernel) reorders cells only
// within an XCD's range.
#define H9G_NXCD 8
__host__ __device__ __forceinline__ unsigned xcd_vwg(unsigned b, unsigned nb) {
  const unsigned x = b % H9G_NXCD, q = nb / H9G_NXCD, r = nb % H9G_NXCD;
  return x * q + (x < r ? x : r) + b / H9G_NXCD;
}

// The tables of the glibc-exact expf/powf (h9_math.h): a device copy per unit
// that includes this header (internal linkage), read into LDS by load_tabs.
static __constant__ uint64_t c_exp2tab[32] = H9M_EXP2F_TAB_INIT;
static __constant__ double c_log2tab[32] = H9M_POWF_LOG2_TAB_INIT;

__device__ __forceinline__ void load_tabs(uint64_t *e2, double *l2) {
  const int t = threadIdx.x;
  if (t < 32) {
    e2[t] = c_exp2tab[t];
    l2[t] = c_log2tab[t];
  }
  __syncthreads();
}

// Pair kernel (h9g_pair.h): two lanes per soil column, the per-layer powers
// split over the pair.  Same arguments, layouts and results as
// h9g_year_kernel.
// Waves per SIMD: 3 at either layer count (h9g_pair.h pair_resident: 168
// VGPRs, 3 x 53 KB LDS per CU at L = 8).
template <int L>
constexpr int pair_waves() { return pair_resident<L>(); }
static_assert(pair_waves<8>() == pair_waves<10>(), "one row of the shape table serves both layer counts");

// The day rows (h9g_set_days) of a cell that does not run its year: NaN on
// each of its nt days, as nan_rows.
static_assert(H9G_NDAYREC == DaysEt::NREC, "the day record of the ABI and of h9g_pair.h");
__device__ __forceinline__ void nan_days(float *base, int nt, size_t n, int c) {
  for (size_t r = 0; r < (size_t)nt * H9G_NDAYREC; r++) base[r * n + c] = __builtin_nanf("");
}

// ---------------------------------------------------------------------------
// kernel kinds and launch shapes
// ---------------------------------------------------------------------------
// Kernel kinds: what a context runs its years on (h9g_ctx::kind, H9G_KERNEL)
// and what a launch ran on (the rows of h9g_launch_stats, which the Python
// layer names: the numbers stay).
enum Kind : int {
  K_PAIR = 1,     // h9g_pair_kernel
  K_SOLO = 2,     // h9g_solo_kernel
  K_MIXED = 3,    // whole rounds of solo waves, then the pair kernel on the rest (l10_kind): two launch ranges
  K_PAIR2 = 4,    // h9g_pair2_kernel (L = 10)
  K_PAIR11 = 5,   // h9g_pair11_kernel
  K_PAIR1 = 6,    // h9g_pair1_kernel, in either shape
  K_PROBE = 7,    // statistics only: the cell order's day-1 probes, whatever kernel ran them
  K_NSTAT         // rows of h9g_ctx::kstat
};

// Launch shapes: what a year launch actually runs on, one row per year kernel.
//   X(id, stem, kind, threads, blocks, cols, waves, pair, g2)
// stem: the kernel is h9g_<stem>_kernel, its monthly sibling h9g_<stem>_mon_kernel,
// its ET sibling h9g_<stem>_et_kernel, its day sibling h9g_<stem>_day_kernel;
// kind: the statistics row it counts under; threads per workgroup; column
// blocks per workgroup; columns per wave (per column block); waves per SIMD =
// workgroups resident per CU (the Pacer's round, pace_mode); pair: a pair
// kernel (day-snapshot blocks, pacing rows); g2: its launches can carry a
// second group of cells (g2_fits).  The kernels' attributes and pair_body
// arguments, the launch's block and grid, the name h9g_kernel_name reports and
// the host's block arithmetic all read the row (shape_info).
// The one-column kernel's two-wave shape is built unless H9G_P1_FRONT=0.
#if H9G_P1_FRONT
#define H9G_SHAPE_PAIR1F(X) X(S_PAIR1F, pair1f, K_PAIR1, 128, 1, 1, 1, true, false)
#else
#define H9G_SHAPE_PAIR1F(X)
#endif
#define H9G_PAIR_SHAPES(X)                                                                      \
  X(S_PAIR, pair, K_PAIR, 64 * H9G_PWAVES, H9G_PWAVES, H9G_PCPW, pair_waves<8>(), true, true)   \
  X(S_PAIR2, pair2, K_PAIR2, 64 * H9G_PWAVES, H9G_PWAVES, H9G_PCPW, 2, true, true)              \
  X(S_PAIR11, pair11, K_PAIR11, 64 * H9G_PWAVES, H9G_PWAVES, H9G_PCPW11, 3, true, true)         \
  X(S_PAIR1, pair1, K_PAIR1, 64 * H9G_PWAVES, H9G_PWAVES, 1, 1, true, false)                    \
  H9G_SHAPE_PAIR1F(X)
#define H9G_YEAR_SHAPES(X) \
  H9G_PAIR_SHAPES(X)       \
  X(S_SOLO, solo, K_SOLO, H9G_YBLOCK, 1, H9G_YBLOCK, 2, false, false)

#define H9G_SHAPE_ID(id, ...) id,
enum Shape : int { H9G_YEAR_SHAPES(H9G_SHAPE_ID) S_NSHAPE };
#undef H9G_SHAPE_ID

struct ShapeInfo {
  const char *name;     // the kernel's name
  const char *et_name;  // its ET sibling's (what an ET context's years run on)
  const char *day_name; // its day sibling's (what a context that records days runs them on)
  Kind kind;
  int threads, blocks, wave_cols, waves;
  bool pair, second_group;
  constexpr int block_cells() const { return blocks * wave_cols; }   // cells per workgroup
  constexpr bool front() const { return threads > 64 * blocks; }     // a second wave per column block (pair_body FRONT)
};
constexpr ShapeInfo shape_info(Shape s) {
  switch (s) {
#define H9G_SHAPE_ROW(id, stem, kind, threads, blocks, cols, waves, pair, g2) \
  case id:                                                                     \
    return {"h9g_" #stem "_kernel", "h9g_" #stem "_et_kernel", "h9g_" #stem "_day_kernel", kind, threads, blocks, cols, \
            waves, pair, g2};
    H9G_YEAR_SHAPES(H9G_SHAPE_ROW)
#undef H9G_SHAPE_ROW
    default: return {};
  }
}
// Workgroups of a launch of `cells` cells (a second group's slots included).
constexpr size_t shape_blocks(Shape s, size_t cells) {
  return (cells + (size_t)shape_info(s).block_cells() - 1) / (size_t)shape_info(s).block_cells();
}
// h9g_pair2_kernel exists at L = 10 only.
constexpr bool shape_at(Shape s, int L) { return s != S_PAIR2 || L == 10; }

// What a kind adds over a shape: its H9G_KERNEL spelling, and the shape its
// pair part, and a list launch of its context, runs as.
struct KindInfo {
  const char *env;
  Shape shape;
};
constexpr KindInfo kind_info(int kind) {
  switch (kind) {
    case K_SOLO: return {"solo", S_SOLO};
    case K_MIXED: return {"mixed", S_PAIR};
    case K_PAIR2: return {"pair2", S_PAIR2};
    case K_PAIR11: return {"pair11", S_PAIR11};
    case K_PAIR1: return {"pair1", S_PAIR1};
    default: return {"pair", S_PAIR};
  }
}

// The shape of a launch of `cells` cells on `kind`, decided here and nowhere
// else: the sort's and the forcing gather's traversal, the grid, the block
// size and the kernel, the monthly dispatch and the name of the kernel that
// ran all follow from it.  The one-column kernel runs a launch of at most
// H9G_PAIR1_FRONT_MAX cells in its two-wave shape, a workgroup per cell
// (h9g_pair1f_kernel: still at most one wave per SIMD); longer lists keep the
// single-wave kernel.
#define H9G_PAIR1_FRONT_MAX 512
inline Shape year_shape(int kind, size_t cells) {
  const Shape s = kind_info(kind).shape;
#if H9G_P1_FRONT
  if (s == S_PAIR1 && cells <= H9G_PAIR1_FRONT_MAX) return S_PAIR1F;
#endif
  return s;
}

// C: columns (pairs) per wave: 22 (h9g_pair_kernel, h9g_pair2_kernel) or 11
// (h9g_pair11_kernel: 42 helper lanes, 2 rounds per phase at L = 10).
// MON: the monthly kernels (month-end snapshots of the running sums into
// `mon`, addressed as a.annual: 12 * annual rows per cell).
// FRONT: the one-column kernel's two-wave shape (h9g_pair.h front_year_pair):
// a workgroup is one column, wave 0 its main wave and wave 1 its front wave,
// both on the column's one LDS block.
// ET: the evapotranspiration kernels (cell_year_pair with EvapProf and
// MonthsEt: row evap of the annual and monthly rows is the year's evaporation
// sum); `mon` may be null there (no monthly recording), a wave-uniform test.
// DAY: the day kernels (h9g_set_days): the ET kernels with the DaysEt policy,
// which stores the day records into `dayr`, addressed as a.annual
// (H9G_NDAYREC rows per day); `dayr` may be null (a day-1 probe).
template <int L, class G, int R, int C = H9G_PCPW, bool MON = false, bool FRONT = false, bool ET = false,
          bool DAY = false>
__device__ __forceinline__ void pair_body(const KArgs &a, const G &g, float *mon = nullptr, float *dayr = nullptr) {
  static_assert(!(MON && ET), "the ET kernels record months themselves");
  static_assert(!DAY || ET, "the day kernels are ET kernels");
  typedef PairStore<L, 2 * C, R, FRONT ? (H9G_P1_SIDE ? 2 : 1) : 0> PS;   // (2: the water-table chain on the second wave too)
  static_assert(!FRONT || C == 1, "the front wave serves a one-column wave");
  constexpr int NW = FRONT ? 1 : H9G_PWAVES;               // column blocks per workgroup
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  __shared__ float s_cell[NW][PS::ROWS * 2 * C];           // [wave][row][lane]
  __shared__ float s_zt[zt_size<L>()];
  // the day snapshot addresses its global block by LDS byte offset
  // (PairStore::svw): every static LDS address must lie inside GBLOCK
  static_assert(sizeof(s_e2) + sizeof(s_l2) + sizeof(s_cell) + sizeof(s_zt) <= (size_t)PS::GBLOCK,
                "pair kernel LDS footprint exceeds the day-snapshot block");
  if (threadIdx.x == 0) fill_zt<L>(g, s_zt);
  load_tabs(s_e2, s_l2);
  const h9m::Tabs T = {s_e2, s_l2};
  const int wave = FRONT ? 0 : threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the front wave runs everything down to the year like the main wave: the
  // same early returns from the same values, and the same values stored to the
  // same words of the block (so it waits for nothing before its first barrier).
  // The reverse must hold too: a front-wave store that lands late must not hit
  // a word the main wave has rewritten meanwhile.  The prologue stores the
  // parameter slots PF_TS..PF_PSI, PS_FMAX, PF_ROOTR and cell_inv_pair's fields
  // (PF_NINVB..PF_RTS1, PS_MH3, PS_TSDZ1); before the first barrier 1 the main
  // wave writes only park's plant state (PS_LAI..), day_consts' PS_DAY and
  // PS_DR* and the HO_* words, and rootr not before the first day's end, many
  // barriers later: the two sets are disjoint.  A field added to either side
  // has to keep them so.
  const bool front_wave = FRONT && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;
  // lanes 0..43: 22 pairs; 44..63: spare lanes, which join the pairs only in
  // the per-layer phases (Split2, hydrology_pair).  Spare lane 44 + j mirrors
  // pair lane 12 + j (mod the wave's pair lanes): its LDS column and
  // starting state, never stored to, so the substep code it runs masked-in
  // stays ordinary; a pure function of the lane, so nothing about it is
  // carried in registers.  Lanes 12..31 because an LDS read's lanes 32..63
  // share one cycle (bank = dword mod 32): their columns' banks are the 20
  // that pair lanes 32..43 leave free, so a mirrored read adds no conflict.
  const bool spare = lane >= 2 * C;
  if (spare && !PS::kSpare) return;
  const int h = lane & 1;
  const int slot0 = __builtin_amdgcn_readfirstlane(
      a.c0 + (int)(xcd_vwg(blockIdx.x, gridDim.x) * NW + wave) * C);
  // the wave's group (wave-uniform: split is a multiple of C)
  const bool g2 = slot0 >= a.split;
  const int lim = g2 ? a.cend : a.bend;
  float *const st = g2 ? a.st2 : a.st;
  int *const err = g2 ? a.err2 : a.err;
  int *const hist = g2 ? nullptr : a.hist;
  const int nt = g2 ? a.nt2 : a.nt;
  const int ncol = min(C, lim - slot0);
  if (ncol <= 0) return;             // an empty wave
  const int pl = spare ? (lane - 2 * C + (C == H9G_PCPW ? 12 : 0)) % (2 * ncol) : lane;
  const int slot = slot0 + (pl >> 1);
  if (slot >= lim) return;           // both lanes of a pair leave together
  const int c = a.perm ? a.perm[slot] : slot;
  const int io = a.sorted_io ? slot : c;   // forcing and annual sums: slot order when sorted
  const int n = a.ncell;
  const size_t ios = a.sorted_io ? a.iostride : (size_t)n;

  int prow, pslot;
  pace_key(prow, pslot);
  PS cs{(lds_float *)&s_cell[wave][pl], (lds_float *)&s_cell[wave][pl & ~1], (const lds_float *)s_zt,
        a.sv + (size_t)blockIdx.x * (PS::GBLOCK / sizeof(float)),
        Pacer{a.pace + (size_t)prow * 16, a.epoch & 0xfffffu, pslot, a.prio_mode,
              (int)((blockIdx.x * (unsigned)PS::RESIDENT) / gridDim.x)},
        (lds_float *)&s_cell[wave][0]};
  const Split2 sp{h, lane, spare};
  St<L> s;
  if (!spare) {
#pragma unroll
    for (int p = PF_TS; p <= PF_PSI; p++)
#pragma unroll
      for (int t = 0; t < L / 2; t++) cs.set_slot(p, t, a.par[(size_t)par_row(L, p, 2 * t + h) * n + c]);
    cs.set_sc(PS_FMAX, a.par[(size_t)Rows<L>::FMAX * n + c]);
#pragma unroll
    for (int t = 0; t < L / 2; t++) cs.set_slot(PF_ROOTR, t, st[(size_t)rootr_row(L, 2 * t + h) * n + c]);
  }
#pragma unroll
  for (int i = 1; i <= L; i++) {
    s.h2o[i] = st[(size_t)(Rows<L>::H2O + i - 1) * n + c];
    s.smp[i] = st[(size_t)(Rows<L>::SMP + i - 1) * n + c];
  }
  H9K_LOAD_SCALARS(L, s, st, n, c)
  cs.launder();

  if (!spare) {
    H9K_TS_SUM(L, cs, ts_sum)
    if (!(ts_sum > SOIL_TRUNC) || err[c] != 0) {
      if (h == 0 && !front_wave) nan_rows(a.annual, Rows<L>::ANNUAL, ios, io);
      if constexpr (MON)
        if (h == 0 && !front_wave) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, io);
      if constexpr (ET)
        if (mon && h == 0 && !front_wave) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, io);
      if constexpr (DAY)
        if (dayr && h == 0 && !front_wave) nan_days(dayr, nt, ios, io);
      return;
    }
    cell_inv_pair<L, G>(g, cs);
  }
  if (__builtin_amdgcn_ballot_w64(!spare) == 0) return;   // every pair masked out: the spare lanes leave too
  if constexpr (FRONT) {
    if (front_wave) {
#if defined(H9G_STAMPS)
      StampProf fp{stamp_clock(), {0, 0, 0, 0, 0, 0, 0, 0}};
      front_year_pair<L, G>(g, cs, sp, T, fp);
      if (lane == 0 && a.stamps)            // the front waves' records follow the main waves'
        for (int k = 0; k < 8; k++) a.stamps[(gridDim.x + blockIdx.x) * 8 + k] = fp.acc[k];
#else
      front_year_pair<L, G>(g, cs, sp, T);
#endif
      return;
    }
  }
  int eday = 0, estep = 0;
  float errval = 0.0f;
#if defined(H9G_STAMPS)
  StampProf pr{stamp_clock(), {0, 0, 0, 0, 0, 0, 0, 0}};
  const int code = cell_year_pair<L, G, Split2, PS, true>(g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, nt,
                                                         a.nisurf, a.grow_on, (gbl_float *)(a.annual + io), ios, eday,
                                                         estep, errval, T, a.raw, pr);
  if (lane == 0 && a.stamps)
    for (int k = 0; k < 8; k++) a.stamps[(blockIdx.x * NW + wave) * 8 + k] = pr.acc[k];
#else
  int code;
  if constexpr (DAY)
    code = cell_year_pair<L, G, Split2, PS, true, EvapProf, DaysEt>(
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, nt, a.nisurf, a.grow_on,
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, EvapProf{zero, g.dt()},
        DaysEt{(gbl_float *)mon, ios, (gbl_float *)dayr, (const gbl_float *)a.annual});
  else if constexpr (ET)
    code = cell_year_pair<L, G, Split2, PS, true, EvapProf, MonthsEt>(
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, nt, a.nisurf, a.grow_on,
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, EvapProf{zero, g.dt()},
        MonthsEt{mon ? (gbl_float *)(mon + io) : nullptr, ios});
  else if constexpr (MON)
    code = cell_year_pair<L, G, Split2, PS, true, NoProf, Months>(
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, nt, a.nisurf, a.grow_on,
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, NoProf(), Months{(gbl_float *)(mon + io), ios});
  else
    code = cell_year_pair<L, G>(g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, nt, a.nisurf,
                                a.grow_on, (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw);
#endif
  if (spare || h != 0) return;       // the even lane writes the cell back
  int cw = c, iow = io;
  opaque(cw);
  opaque(iow);
  cs.launder();
  if (hist) hist[cw] = s.naq;
  H9K_STORE_CELL(L, s, cs, st, n, cw, a.grow_on, SC_N)
  if (code) {
    stop_write(err, n, cw, code, eday, estep, errval, a.err_flag);
    nan_rows(a.annual, Rows<L>::ANNUAL, ios, iow);
    if constexpr (MON) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, iow);
    if constexpr (ET)
      if (mon) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, iow);
  }
}

// The pair kernels, one per row of H9G_PAIR_SHAPES, each with its monthly
// sibling (h9g_set_monthly): the same body under a name of its own, with the
// Months policy of cell_year_pair and the base of the monthly rows as an
// argument after KArgs -- KArgs itself is the same, so the plain kernels keep
// their argument layout and their machine code.  The monthly kernels are
// launched only by a context with monthly recording on, never by a probe.
// And each with its ET sibling (h9g_set_evap), the same way: EvapProf and
// MonthsEt, `mon` null without monthly recording.  An ET context runs every
// year launch on them, its day-1 probes included.
// And each with its day sibling (h9g_set_days): EvapProf and DaysEt, the base
// of the day rows an argument after `mon`.  A context that records days runs
// its years on them; its day-1 probes stay on the ET kernels.
//   * pair2: the pair kernel built for 2 waves per SIMD (round 4, VERDICT r03
//     #2/#4): 256 VGPRs, so the L = 10 substep does not spill (the 3-wave build
//     spills 108 VGPRs and 118 SGPRs into a 296-B-per-lane scratch that reaches
//     HBM), and 80 KB of LDS per workgroup, so every reciprocal field fits.  It
//     trades a third of the resident waves for that; l10_kind picks it by
//     shard size.
//   * pair11: 11 columns per wave (round 5): the 42 lanes past
//     the pairs help in the per-layer phases, which then take 2 rounds instead
//     of 5 at L = 10 (hydrology_pair helpers), and the wave's LDS block halves,
//     so every reciprocal field fits at 3 waves per SIMD.  Twice the waves of
//     22-column ones for the same cells.  Measured on the 8-GPU config-5 shard
//     (33,750 cells: 3,069 waves for 3,072 slots) it lost to pair2 (DESIGN.md
//     §6), so l10_kind never picks it; H9G_KERNEL=pair11 selects it, and the
//     GPU tests run it.
//   * pair1: one column per wave (round 5): the 62 lanes past the pair help in
//     the per-layer phases, which take one round each (hydrology_pair
//     helpers), and the wave may hold every register (one wave per SIMD: no
//     spills).  For the short lists of the cell-order re-runs
//     (h9g_run_decade_ordered), whose years run as lone waves: a lone wave's
//     year is latency-bound, and this cuts its per-layer rounds from 3 to 1 at
//     L = 8 (from 5 to 1 at L = 10).  Round 7: its powers of the per-layer
//     phases, the single-power round and the aquifer node run as two task
//     rounds, a power per lane (hydrology_pair kTask).
//   * pair1f: its two-wave shape (round 9): a workgroup is one column, whose
//     second wave evaluates the front of each substep beside the first wave's
//     per-layer rounds (h9g_pair.h front_year_pair).  Twice the waves per
//     cell, one per SIMD still (year_shape).
#define H9G_YEAR_ATTRS(id)                  \
  __launch_bounds__(shape_info(id).threads) \
      __attribute__((amdgpu_waves_per_eu(shape_info(id).waves, shape_info(id).waves)))
#define H9G_PAIR_KERNELS(id, stem, ...)                                                                          \
  template <int L, class G>                                                                                      \
  __global__ void H9G_YEAR_ATTRS(id) h9g_##stem##_kernel(const KArgs a, const G g) {                             \
    pair_body<L, G, shape_info(id).waves, shape_info(id).wave_cols, false, shape_info(id).front()>(a, g);        \
  }                                                                                                              \
  template <int L, class G>                                                                                      \
  __global__ void H9G_YEAR_ATTRS(id) h9g_##stem##_mon_kernel(const KArgs a, float *mon, const G g) {             \
    pair_body<L, G, shape_info(id).waves, shape_info(id).wave_cols, true, shape_info(id).front()>(a, g, mon);    \
  }                                                                                                              \
  template <int L, class G>                                                                                      \
  __global__ void H9G_YEAR_ATTRS(id) h9g_##stem##_et_kernel(const KArgs a, float *mon, const G g) {              \
    pair_body<L, G, shape_info(id).waves, shape_info(id).wave_cols, false, shape_info(id).front(), true>(a, g,   \
                                                                                                        mon);   \
  }                                                                                                              \
  template <int L, class G>                                                                                      \
  __global__ void H9G_YEAR_ATTRS(id) h9g_##stem##_day_kernel(const KArgs a, float *mon, float *day, const G g) { \
    pair_body<L, G, shape_info(id).waves, shape_info(id).wave_cols, false, shape_info(id).front(), true, true>(  \
        a, g, mon, day);                                                                                         \
  }
H9G_PAIR_SHAPES(H9G_PAIR_KERNELS)
#undef H9G_PAIR_KERNELS

// Solo kernel: one lane per soil column running the generic code of
// h9g_pair.h with one lane doing every layer (SplitAll: two layers per
// scheduling region, tridiagonal rows eliminated as assembled).
// The body is a macro, expanded in place in the kernel and in its monthly
// sibling (MON, `mon`: pair_body's): as an inlined function the same
// statements compiled to other machine code for the kernel (blockDim.x loaded
// from the dispatch packet; as with the row macros of h9g_rows.h).  ET: the
// ET sibling (pair_body's; its store has the snapshot field SV_EVAP).  DAY,
// dayr: the day sibling (pair_body's).
#define H9G_SOLO_BODY(MON, ET, mon, DAY, dayr)                                                                     \
  typedef SoloStore<L, ET> SS;                                                                                     \
  __shared__ uint64_t s_e2[32];                                                                                    \
  __shared__ double s_l2[32];                                                                                      \
  __shared__ float s_cell[SS::ROWS * H9G_YBLOCK];                                                                  \
  __shared__ float s_zt[zt_size<L>()];                                                                             \
  if (threadIdx.x == 0) fill_zt<L>(g, s_zt);                                                                       \
  load_tabs(s_e2, s_l2);                                                                                           \
  const h9m::Tabs T = {s_e2, s_l2};                                                                                \
  const int slot = a.c0 + (int)(xcd_vwg(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x);                        \
  if (slot >= a.cend) return;                                                                                      \
  const int c = a.perm ? a.perm[slot] : slot;                                                                      \
  const int io = a.sorted_io ? slot : c;                                                                           \
  const int n = a.ncell;                                                                                           \
  const size_t ios = a.sorted_io ? a.iostride : (size_t)n;                                                         \
  SS cs{(lds_float *)&s_cell[threadIdx.x], (const lds_float *)s_zt};                                               \
  const SplitAll sp;                                                                                               \
  St<L> s;                                                                                                         \
  H9K_LOAD_LANE(L, cs, s, a.par, n, c, a.st, n, c)                                                                 \
  H9K_LOAD_SCALARS(L, s, a.st, n, c)                                                                               \
  cs.launder();                                                                                                    \
  H9K_TS_SUM(L, cs, ts_sum)                                                                                        \
  if (!(ts_sum > SOIL_TRUNC) || a.err[c] != 0) {                                                                   \
    nan_rows(a.annual, Rows<L>::ANNUAL, ios, io);                                                                  \
    if constexpr (MON) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, io);                                      \
    if constexpr (ET)                                                                                              \
      if (mon) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, io);                                              \
    if constexpr (DAY)                                                                                             \
      if (dayr) nan_days(dayr, a.nt, ios, io);                                                                     \
    return;                                                                                                        \
  }                                                                                                                \
  cell_inv_pair<L, G>(g, cs);                                                                                      \
  int eday = 0, estep = 0;                                                                                         \
  float errval = 0.0f;                                                                                             \
  int code;                                                                                                        \
  if constexpr (DAY)                                                                                               \
    code = cell_year_pair<L, G, SplitAll, SS, false, EvapProf, DaysEt>(                                            \
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, a.nt, a.nisurf, a.grow_on,                    \
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, EvapProf{zero, g.dt()},                  \
        DaysEt{(gbl_float *)mon, ios, (gbl_float *)dayr, (const gbl_float *)a.annual});                            \
  else if constexpr (ET)                                                                                           \
    code = cell_year_pair<L, G, SplitAll, SS, false, EvapProf, MonthsEt>(                                          \
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, a.nt, a.nisurf, a.grow_on,                    \
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, EvapProf{zero, g.dt()},                  \
        MonthsEt{mon ? (gbl_float *)(mon + io) : nullptr, ios});                                                   \
  else if constexpr (MON)                                                                                          \
    code = cell_year_pair<L, G, SplitAll, SS, false, NoProf, Months>(                                              \
        g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar, a.nt, a.nisurf, a.grow_on,                    \
        (gbl_float *)(a.annual + io), ios, eday, estep, errval, T, a.raw, NoProf(),                                \
        Months{(gbl_float *)(mon + io), ios});                                                                     \
  else                                                                                                             \
    code = cell_year_pair<L, G, SplitAll, SS, false>(g, cs, sp, s, (const gbl_float *)(a.forc + io), ios, a.fvar,  \
                                                     a.nt, a.nisurf, a.grow_on, (gbl_float *)(a.annual + io), ios, \
                                                     eday, estep, errval, T, a.raw);                               \
  int cw = c, iow = io;                                                                                            \
  opaque(cw);                                                                                                      \
  opaque(iow);                                                                                                     \
  cs.launder();                                                                                                    \
  if (a.hist) a.hist[cw] = s.naq;                                                                                  \
  H9K_STORE_CELL(L, s, cs, a.st, n, cw, a.grow_on, SC_N)                                                           \
  if (code) {                                                                                                      \
    stop_write(a.err, n, cw, code, eday, estep, errval, a.err_flag);                                               \
    nan_rows(a.annual, Rows<L>::ANNUAL, ios, iow);                                                                 \
    if constexpr (MON) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, iow);                                     \
    if constexpr (ET)                                                                                              \
      if (mon) nan_rows(mon, H9G_NMONTHS * Rows<L>::ANNUAL, ios, iow);                                             \
  }

template <int L, class G>
__global__ void H9G_YEAR_ATTRS(S_SOLO) h9g_solo_kernel(const KArgs a, const G g) {
  H9G_SOLO_BODY(false, false, ((float *)nullptr), false, ((float *)nullptr))
}
template <int L, class G>
__global__ void H9G_YEAR_ATTRS(S_SOLO) h9g_solo_mon_kernel(const KArgs a, float *mon, const G g) {
  H9G_SOLO_BODY(true, false, mon, false, ((float *)nullptr))
}
template <int L, class G>
__global__ void H9G_YEAR_ATTRS(S_SOLO) h9g_solo_et_kernel(const KArgs a, float *mon, const G g) {
  H9G_SOLO_BODY(false, true, mon, false, ((float *)nullptr))
}
template <int L, class G>
__global__ void H9G_YEAR_ATTRS(S_SOLO) h9g_solo_day_kernel(const KArgs a, float *mon, float *day, const G g) {
  H9G_SOLO_BODY(false, true, mon, true, day)
}

// ---------------------------------------------------------------------------
// geometry dispatch and the year launch
// ---------------------------------------------------------------------------
// Kernel variant for a configuration: compile-time geometry when zi is one of
// the built-in layer sets and NISURF is 24 or 48, runtime geometry otherwise.
enum GeoKind { GEO_R = 0, GEO_C24 = 24, GEO_C48 = 48 };

inline GeoKind geo_kind(const h9g_config &c) {
  const float *zd = c.nlayers == 8 ? ZiDefault<8>::zi : ZiDefault<10>::zi;
  for (int i = 0; i <= c.nlayers + 1; i++)
    if (c.zi[i] != zd[i]) return GEO_R;
  if (c.nisurf == 24) return GEO_C24;
  if (c.nisurf == 48) return GEO_C48;
  return GEO_R;
}

// f(L, g) with the configuration's layer count as a compile-time constant (a
// std::integral_constant: `L` is a template argument in f) and its geometry
// object, GeoC<L, 48>, GeoC<L, 24> or GeoR<L>; returns what f returns.  A
// generic lambda at each call site names its kernel K<L, decltype(g)>.
template <class F>
int geo_dispatch(const h9g_config &cfg, F &&f) {
  const GeoKind gk = geo_kind(cfg);
#if defined(H9G_ONLY_C2)
  // A/B measurement builds (tools/build_variant.py --c2): the driver's config-2
  // instantiation only (L = 8, driver.txt layers, NISURF = 48), ~1 minute
  // instead of ~4 to build; any other configuration is refused.
  if (cfg.nlayers != 8 || gk != GEO_C48) {
    fprintf(stderr, "h9g: H9G_ONLY_C2 build runs config 2 only\n");
    return H9G_EINVAL;
  }
  return f(std::integral_constant<int, 8>(), GeoC<8, 48>());
#else
  auto at = [&](auto L) {
    if (gk == GEO_C48) return f(L, GeoC<L, 48>());
    if (gk == GEO_C24) return f(L, GeoC<L, 24>());
    return f(L, make_geo_r<L>(cfg.zi, cfg.nisurf));
  };
  return cfg.nlayers == 8 ? at(std::integral_constant<int, 8>()) : at(std::integral_constant<int, 10>());
#endif
}

// The year kernel of `shape` -- V_MON: its monthly sibling, with `mon` the
// base of the launch's monthly rows; V_ET: its ET sibling, `mon` the same or
// null; V_DAY: its day sibling, `mon` as V_ET's and `day` the base of the
// launch's day rows -- over a's slots [c0, cend), with the configuration's
// geometry variant.  The plain case is h9g_plain_launch of h9g_plain.hip, the
// monthly case h9g_mon_launch of h9g_mon.hip, the ET case h9g_et_launch of
// h9g_et.hip and the day case h9g_day_launch of h9g_day.hip, so each unit
// compiles only its own kernels.
enum Variant : int { V_PLAIN = 0, V_MON, V_ET, V_DAY };
template <Variant V>
int launch_shape(Shape shape, const h9g_config &cfg, hipStream_t stream, const KArgs &a, float *mon,
                 float *day = nullptr) {
  const unsigned grid = (unsigned)shape_blocks(shape, (size_t)(a.cend - a.c0)), block = (unsigned)shape_info(shape).threads;
  return geo_dispatch(cfg, [&](auto L, auto g) {
    switch (shape) {
#define H9G_SHAPE_CASE(id, stem, ...)                                                              \
  case id:                                                                                         \
    if constexpr (!shape_at(id, L)) return (int)H9G_EINVAL;                                        \
    else if constexpr (V == V_DAY) h9g_##stem##_day_kernel<L, decltype(g)><<<grid, block, 0, stream>>>(a, mon, day, g); \
    else if constexpr (V == V_ET) h9g_##stem##_et_kernel<L, decltype(g)><<<grid, block, 0, stream>>>(a, mon, g); \
    else if constexpr (V == V_MON) h9g_##stem##_mon_kernel<L, decltype(g)><<<grid, block, 0, stream>>>(a, mon, g); \
    else h9g_##stem##_kernel<L, decltype(g)><<<grid, block, 0, stream>>>(a, g);                    \
    return 0;
      H9G_YEAR_SHAPES(H9G_SHAPE_CASE)
#undef H9G_SHAPE_CASE
      default: return (int)H9G_EINVAL;
    }
  });
}

// ---------------------------------------------------------------------------
// the kernel units' host side: what the host runtime (h9g_ctx.h) calls
// ---------------------------------------------------------------------------
// h9g_plain.hip: launch_shape<V_PLAIN>.  h9g_mon.hip: launch_shape<V_MON>, and
// the cell order's NaN recorded rows of the cells that start a decade stopped.
// h9g_et.hip: launch_shape<V_ET>.  h9g_day.hip: launch_shape<V_DAY>.
int h9g_plain_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a);
int h9g_mon_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon);
int h9g_et_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon);
int h9g_day_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon, float *day);
int h9g_nan_stopped_rows(int n, int rows, const int *err0, float *dst, hipStream_t stream);

// Not exported from libh9g.so.
#define H9G_LOCAL __attribute__((visibility("hidden")))

#define HIPCHK(x)                                                              \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "h9g: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), \
              __FILE__, __LINE__);                                             \
      return H9G_EHIP;                                                         \
    }                                                                          \
  } while (0)

// h9g_cols.hip: the one-lane-per-column kernels, each behind a launcher that
// picks the configuration's geometry variant (geo_dispatch) and its grid.
#define H9G_BLOCK 256   // threads per block of the per-cell helper kernels

// h9g_site_kernel's arguments.  Parameters and state as the year kernels.
struct SiteArgs {
  int ncell, nday, nisurf;
  const float *__restrict__ par;
  float *__restrict__ st;
  const float *__restrict__ sub, *__restrict__ daily, *__restrict__ lai;
  float *__restrict__ out;
  int *__restrict__ err;
  int *__restrict__ err_flag;
};

// h9g_focus_kernel's arguments.
struct FocusArgs {
  int ncell, nsel, nyears, nisurf, grow_on;
  size_t fvar;
  const float *__restrict__ par;
  const float *__restrict__ st;
  const int *__restrict__ sel;
  const int *__restrict__ err;     // the cells' STOP records when the run starts (rows of ncell)
  const FocusYear *__restrict__ yrs;
  float *__restrict__ out;
};

// h9g_init_kernel over the ncell cells: the reference's initial state from par.
H9G_LOCAL int h9g_init_launch(const h9g_config *cfg, hipStream_t stream, int ncell, const float *par, float *st);
// h9g_sort_kernel over slots [c0, cend) in workgroups of cpb cells, of the
// cells `list` (null: the slots' own numbers) with state st and STOP rows err,
// by the sort history hist over nsub substeps, into perm.
H9G_LOCAL int h9g_sort_launch(const h9g_config *cfg, hipStream_t stream, int n, int c0, int cend, int cpb,
                              const float *st, const int *err, const int *hist, int nsub, int *perm,
                              const int *list);
H9G_LOCAL int h9g_site_launch(const h9g_config *cfg, hipStream_t stream, const SiteArgs &a);
H9G_LOCAL int h9g_focus_launch(const h9g_config *cfg, hipStream_t stream, const FocusArgs &a);

// Measurement builds.  Their device globals (h9g_step.h, h9g_pair.h) exist
// once per unit; these read and write the copies of h9g_plain.hip, the unit
// whose kernels the measurement builds run (tools/build_variant.py).  The
// monthly and ET kernels count into their own units' copies, as before the
// plain kernels had a unit of their own; so do now h9g_site_kernel and
// h9g_focus_kernel (h9g_cols.hip), whose substeps pass the same H9G_BR sites
// and once shared the plain kernels' copy.  No copy but h9g_plain.hip's is
// read or cleared: a count covers the plain year kernels alone.
#if defined(H9G_COUNT_EXACT)
H9G_LOCAL int h9g_exact_report(void);    // prints the exact re-run counts
#endif
#if defined(H9G_COUNT_BRANCH)
H9G_LOCAL int h9g_branch_report(void);   // prints the branch counts since the last call, and clears them
#endif
#if defined(H9G_DUMP_AQ)
H9G_LOCAL int h9g_aq_set(unsigned *bits, const float *base, hipStream_t stream);   // h9g_aq_bits, h9g_aq_base
#endif
