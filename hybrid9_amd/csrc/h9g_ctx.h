// h9g_ctx.h -- what the host runtime's units share (not ABI): the context,
// the description of a recorded output (RecStream) and of a year launch
// (YearSpec), and the few functions that cross units.
// Included by h9g.hip (context, forcing, the year launch, recording),
// h9g_ord.hip (the ordered mode), h9g_spin.hip (spin-up), h9g_stat.hip (day
// statistics), h9g_quant.hip (day quantiles) and h9g_aux.hip (soil build, synthetic inputs, self-tests).  The kernel units (h9g_plain.hip, h9g_mon.hip,
// h9g_et.hip, h9g_day.hip, h9g_cols.hip) do not include it: a change here recompiles no
// geometry-templated kernel.  Their launchers are declared in h9g_year.h.
#pragma once
#include <stdint.h>

#include <string>
#include <thread>
#include <vector>

#include "h9g_year.h"

#define NEVT 64
static inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

static inline int days_in_year(int y) {   // INIT.f90:844-859
  if (y % 4 != 0) return 365;
  if (y % 100 != 0) return 366;
  if (y % 400 != 0) return 365;
  return 366;
}

static inline unsigned nblocks(size_t n) { return (unsigned)((n + H9G_BLOCK - 1) / H9G_BLOCK); }

// One recorded per-cell output beside the annual means: a year kernel writes
// it as rows of n addressed as the annual rows are (d_ann / d_ann_s), every
// year launch passes its destinations beside the annual ones (YearSpec), and
// the ordered mode keeps it per decade beside the annual means (OrdDec::rec)
// and per call in a retained buffer.  Two streams: a year's month-end
// snapshots, 12 x annual rows; and its day records, H9G_NDAYREC rows a day at
// max_days a year, so that a year's rows lie at the same place whatever its
// length.  The streams differ in those two row counts (h9g_create) and in
// nothing else.
enum { REC_MON, REC_DAY, REC_N };
struct RecStream {
  int on = 0;                     // recording on
  size_t year_rows = 0;           // rows of n a year occupies
  int day_rows = 0;               // rows each day of a year writes; 0: every year writes all year_rows
  float *d_year = nullptr;        // a year's rows (as d_ann; NaN until a year writes them)
  float *d_year_s = nullptr;      // ... in slot order (as d_ann_s)
  float *d_ret = nullptr;         // an ordered call's years, (years, year_rows, n)
  size_t ret_cap = 0;             // years allocated there
  int base = 0;                   // first year of the running ordered call there
  std::vector<int> nt;            // days of each year recorded by the last call (empty: none)
  bool in_ret = false;            // ... in d_ret (an ordered call) or d_year (h9g_run_year)
  size_t year_floats(size_t n) const { return year_rows * n; }
  size_t rows_written(int days) const { return day_rows ? (size_t)days * day_rows : year_rows; }
  float *ret_year(size_t n, int k) const { return d_ret + (size_t)k * year_floats(n); }
};
// Every buffer of a recording: H9G_ENOMEM where it does not fit (include/h9g.h).
static inline int rec_malloc(float **p, size_t floats) {
  if (hipMalloc(p, sizeof(float) * floats) == hipSuccess) return 0;
  (void)hipGetLastError();
  *p = nullptr;
  return H9G_ENOMEM;
}

struct h9g_ctx {
  h9g_config cfg;
  int device = 0;
  int L = 8;
  size_t n = 0;
  hipStream_t sc = nullptr, sx = nullptr;      // compute, copy
  float *d_par = nullptr, *d_st = nullptr, *d_forc = nullptr, *d_ann = nullptr;
  int *d_err = nullptr, *d_errflag = nullptr;
  double *d_diag = nullptr;
  int64_t *d_gid = nullptr;
  float *d_lat = nullptr;
  std::vector<int> slot_days;
  std::vector<hipEvent_t> ev_copied, ev_consumed;
  hipEvent_t ev0[NEVT], ev1[NEVT];
  hipEvent_t ev_ext = nullptr, ev_diag = nullptr;   // h9g_get_diagnostics_async ordering
  int nev = 0;
  float last_ms = 0.0f;
  double total_ms = 0.0;
  int last_year = 0;
  int params_set = 0, state_set = 0, ran = 0;
  h9g_error last_err{};
  std::string kname;              // the year kernel's name (year_kernel_name)
  unsigned *d_stamps = nullptr;   // H9G_STAMPS builds only
  std::vector<int64_t> h_gid;     // grid ids of the cells (h9g_set_cells), for NetCDF ingest
  std::vector<float *> h_pin;     // per-slot pinned staging of the NetCDF prefetch
  std::vector<std::thread> prefetch;
  std::vector<int> prefetch_rc;
  unsigned soil_layers = 0;       // layers built by h9g_soil_layer (bit i = layer i)
  float soil_ms = 0.0f;           // device time of the last h9g_soil_layer
  int soil_slow = 0;              // cells of the last layer summed in the reference's order
  int *d_slow = nullptr;
  float *d_sv = nullptr;          // pair kernel day-snapshot blocks
  int *d_perm = nullptr;          // cell order of the year kernel (h9g_sort_kernel)
  int *d_perm2 = nullptr;         // a launch's second group as listed (sorted into d_perm)
  float *d_forc_s = nullptr;      // the year's forcing in slot order (h9g_perm_forcing_kernel)
  float *d_ann_s = nullptr;       // the year kernel's annual sums in slot order
  unsigned *d_aqbits = nullptr;   // H9G_DUMP_AQ builds: day-level water-table record of the last year
  int64_t dec_stats[4] = {0, 0, 0, 0};   // last h9g_run_decade_ordered (h9g_decade_stats)
  std::vector<int> chain_id;      // h9g_set_chains: reference rank (block) of every cell; empty = one chain
  std::vector<int64_t> dec_launches;   // last h9g_run_decade_ordered: cells of each re-run launch
  int *d_hist = nullptr;          // per cell: substeps of the last year below the column (-1: none)
  int hist_nsub = 0;              // substeps of that year
  unsigned *d_pace = nullptr;     // Pacer mode 2 progress rows (h9g_pair.h)
  unsigned epoch = 0;
  int prio_mode = -1;             // H9G_PRIO: 0 none, 1 rotate, 2 pace; -1 auto (pace_mode)
  int ncu = 256;
  int sort = 1;                   // H9G_SORT=0: identity order
  size_t sv_bytes = 0;
  Kind kind = K_PAIR;  // H9G_KERNEL=pair|solo|mixed|pair2|pair11|pair1; default by L and the shard size, l10_kind
  size_t n_solo = 0;   // K_MIXED: cells [0, n_solo) run on the solo kernel, the rest on the pair kernel
  size_t ios = 0;      // slots of the slot-ordered buffers (d_perm, d_forc_s, d_ann_s): twice the cells
  size_t stamp_words = 0;
  Shape stamp_shape = S_PAIR;     // the last stamped launch: its shape ...
  size_t stamp_blocks = 0;        // ... and its grid (the front waves' records follow the grid's main waves')
  int ev_kind[NEVT] = {};         // kernel kind and cell-years of each timed launch
  int64_t ev_cells[NEVT] = {};
  double kstat[K_NSTAT][3] = {};        // per kernel kind: launches, cell-years, ms (h9g_launch_stats)
  struct OrdBufs *ord = nullptr;  // h9g_run_ordered's decade buffers
  int64_t ord_stats[9] = {};      // last ordered call (h9g_ordered_stats)
  int ord_probe = 1;              // the checks' day-1 probe (H9G_NO_PROBE: off)
  // the other switches h9g_create reads from the environment: list launches
  // never on the one-column / 11-column kernel (H9G_NO_PAIR1, H9G_NO_PAIR11),
  // the ordered mode's first passes with every cell (H9G_NO_EXCLUDE) and
  // without riding re-runs (H9G_NO_RIDE)
  int no_pair1 = 0, no_pair11 = 0, no_exclude = 0, no_ride = 0;
  std::vector<int64_t> ord_passes;
  // daily diagnostics (h9g_set_daily / h9g_get_daily; h9g_focus_kernel)
  std::vector<int> daily_sel;     // the selected cells; empty: off
  int *d_dsel = nullptr;          // ... on the device
  float *d_dst = nullptr;         // their gathered start state, state rows of nsel
  float *d_daily = nullptr;       // the lines of the last call, (days, 11, nsel)
  size_t daily_cap = 0;           // floats allocated there
  FocusYear *d_fyrs = nullptr;    // a launch's years (forcing base, days)
  size_t fyrs_cap = 0;
  std::vector<FocusYear> h_fyrs;
  std::vector<int> daily_nt;      // days of each year recorded by the last call
  // the recorded per-cell outputs (RecStream): months (h9g_set_monthly /
  // h9g_get_monthly; the monthly kernels) and day records (h9g_set_days /
  // h9g_get_days; the day kernels; on only with evap on)
  RecStream rec[REC_N];
  bool recording() const { return rec[REC_MON].on || rec[REC_DAY].on; }
  // evapotranspiration output (h9g_set_evap; the ET kernels): row evap of the
  // annual and monthly rows is the year's evaporation sum.  No buffer of its own.
  int evap = 0;
  struct SpinBufs *spin = nullptr;   // h9g_spinup's buffers (h9g_spin.hip); null until its first call
  struct StatBufs *stat = nullptr;   // h9g_get_daystats' result buffer (h9g_stat.hip); null until its first call
  struct QuantBufs *quant = nullptr; // h9g_get_dayquant's result buffer (h9g_quant.hip); null until its first call
};

// One year launch (run_year_impl).
struct YearSpec {
  int slot = 0, jyear = 0;
  const int *d_list = nullptr;   // null: every cell, in h9g_sort_kernel's order; else the m cells d_list[0..m)
  int m = 0;
  float *ann_dst = nullptr;      // list launches: their annual means into these rows (stride n, cell order)
  float *rec_dst[REC_N] = {};    // ... and the rows of every recording that is on into these
  float *st = nullptr;           // the cells' state and STOP rows (null: the context's own)
  int *err = nullptr;
  bool bulk = false;             // a list launch that is a year of the context's cells (h9g_run_ordered's
                                 // first pass without the cells still re-running the decade before): the
                                 // context's kernel, sort history and diagnostics, as an every-cell launch
  // launches of a pair kernel (g2_fits): a second group of the k2 cells
  // h2[0..k2) (host) at year jyear2 from slot2, with state st2/err2, annual
  // means into ann2 and the rows of every recording that is on into rec2
  // (h9g_run_ordered: a decade's re-runs riding in the next decade's years)
  const int *h2 = nullptr;
  int k2 = 0, slot2 = 0, jyear2 = 0;
  float *st2 = nullptr, *ann2 = nullptr, *rec2[REC_N] = {};
  int *err2 = nullptr;
  // list launches: only the year's first `ndays` days (0: all), the annual
  // rows as undivided running sums (the cell order's day-1 probe)
  int ndays = 0;
  bool probe = false;
};

// The functions that cross the host units (hidden: libh9g.so exports the ABI
// of include/h9g.h only; C linkage as their definitions stand among the ABI's).
extern "C" {
// h9g.hip
H9G_LOCAL int run_year_impl(h9g_ctx *ctx, const YearSpec &ys);
H9G_LOCAL bool g2_fits(const h9g_ctx *ctx, size_t base, size_t k);
H9G_LOCAL int fold_events(h9g_ctx *ctx);
H9G_LOCAL int join_prefetch(h9g_ctx *ctx, int slot);
H9G_LOCAL int daily_begin(h9g_ctx *ctx, int jyear0, int nyears);
H9G_LOCAL int daily_launch(h9g_ctx *ctx, const float *st, const float *guess, const int *err, const int32_t *slots,
                           int jyear0, int ny);
H9G_LOCAL int rec_begin(h9g_ctx *ctx, int nyears);
H9G_LOCAL int diag_launch(h9g_ctx *ctx);
// h9g_ord.hip
H9G_LOCAL void ord_free(h9g_ctx *ctx);
// h9g_spin.hip
H9G_LOCAL void spin_free(h9g_ctx *ctx);
// h9g_stat.hip
H9G_LOCAL void stat_free(h9g_ctx *ctx);
// h9g_quant.hip
H9G_LOCAL void quant_free(h9g_ctx *ctx);
}
