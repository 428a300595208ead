/*
 * h9g.h -- C-ABI of the MI355X HYBRID9 hot path (libh9g.so).
 *
 * Replaces the PGF cell loop of the reference driver
 *   /root/reference/SOURCE/HYBRID9.f90:120-295   (cell -> year -> day ->
 *   substep loop calling HYDROLOGY at :203 and GROW at :217)
 * which has no plugin/FFI surface of its own: HYDROLOGY and GROW take no
 * arguments and communicate through MODULE SHARED / CONTROL globals
 * (/root/reference/SOURCE/HYDROLOGY.f90:10-11, GROW.f90:11-12).  One call
 * of h9g_run_year advances every cell of a context through one calendar
 * year, exactly as one pass of HYBRID9.f90:130-291 does for one cell.
 *
 * Plain pointers and sizes only.  Host arrays use the reference's
 * Fortran layouts (SHARED.f90), with the land cells of a block compacted
 * into one dimension:
 *   per-layer arrays   A(L, ncell)     layer fastest   (SHARED.f90:398-429)
 *   per-cell arrays    A(ncell)                        (SHARED.f90:446-472)
 *   forcing            F(ncell, nday)  cell fastest, one array per variable
 *                      in READ_PGF.f90 order: tas rlds rsds huss ps pr rhs
 * The fortran/h9_gpu.f90 module binds every entry point with BIND(C).
 *
 * Semantics: h9g_run_decade_ordered is bit-identical to the reference as
 * it runs on one rank (its cells in order, the module array smp of
 * SHARED.f90:198 carried from cell to cell); h9g_run_year runs isolated
 * cells (every cell carries its own smp), bit-identical to the reference
 * harness run that way.
 * Threading: one host thread per context; contexts are not re-entrant;
 * one context per GPU.  All calls return 0 on success, a positive
 * H9G_ERR_* code for a reference STOP condition (details via
 * h9g_last_error) or a negative H9G_E* code for API/HIP failures.
 */
#ifndef H9G_H
#define H9G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H9G_ABI_VERSION 1
#define H9G_LMAX 10          /* soil layers supported: 8 (reference) or 10 */
#define H9G_NFORCING 7
#define H9G_NANNUAL_SCALARS 11
#define H9G_NDIAG 12
#define H9G_MAX_SLOTS 512   /* forcing slots per context; HBM bounds it too */

/* reference STOP sites (HYDROLOGY.f90) */
#define H9G_ERR_TRIDIAG1 1   /* :806-812  bmx(1) == 0            */
#define H9G_ERR_TRIDIAG2 2   /* :818-825  zero pivot             */
#define H9G_ERR_RSUB_POS 3   /* :1068-1072 rsub_top_tot > 0      */
#define H9G_ERR_IMBALANCE 4  /* :1244-1274 |w1 - w0| > 0.1 mm    */
/* not a reference STOP: the pair kernel's exact re-run was requested in a
 * substep with no day snapshot to replay from (an internal invariant,
 * DESIGN.md §3 "Day snapshot"; never raised by a correct build) */
#define H9G_ERR_NOSNAP 5
/* API / runtime failures */
#define H9G_EINVAL (-1)
#define H9G_EHIP (-2)
#define H9G_ENOMEM (-3)
#define H9G_ESTATE (-4)

typedef struct h9g_ctx h9g_ctx;

typedef struct {
  int32_t ncell;       /* land cells owned by this context (shard)          */
  int32_t nlayers;     /* L: 8 or 10 (SHARED.f90:294 nsoil_layers_max)      */
  int32_t nisurf;      /* substeps per day (driver.txt line 2, INIT.f90:183) */
  int32_t grow_on;     /* 1: CALL GROW daily (HYBRID9.f90:217); 0: frozen   */
  int32_t max_days;    /* forcing slot capacity in days (>= 366)            */
  int32_t nslots;      /* forcing slots (2 = double-buffered prefetch; up to
                          H9G_MAX_SLOTS resident years, bounded by free HBM) */
  float zi[H9G_LMAX + 2]; /* zi(0:L+1) mm (driver.txt:17-26, INIT.f90:202)  */
} h9g_config;

typedef struct {
  int32_t code;        /* H9G_ERR_* of the first failing cell (0: none)     */
  int32_t cell;        /* its 0-based index in the context                  */
  int32_t year;        /* calendar year                                     */
  int32_t day;         /* 0-based day of year (DOY-1)                       */
  int32_t substep;     /* 0-based NS-1                                      */
  float value;         /* w1-w0, pivot row, rsub_top_tot ...               */
} h9g_error;

/* --- lifetime -------------------------------------------------------- */
int h9g_abi_version(void);
int h9g_device_count(void);
/* Host-only validation of a configuration (needs no GPU): 0, or H9G_EINVAL
 * with a NUL-terminated reason in `reason` (may be NULL). */
int h9g_config_check(const h9g_config *cfg, char *reason, int reason_len);
/* Device bytes a context of this configuration allocates (0 if invalid). */
size_t h9g_config_bytes(const h9g_config *cfg);
/* Creates a context on HIP device `device`; NULL on failure, with the
 * reason (invalid field, free HBM short of h9g_config_bytes, no device)
 * in h9g_create_error() of the calling thread. */
h9g_ctx *h9g_create(const h9g_config *cfg, int device);
const char *h9g_create_error(void);
void h9g_destroy(h9g_ctx *ctx);

/* --- parameters and state (INIT.f90) ---------------------------------- */
/* theta_s, hksat, bsw, psi_s: (L, ncell); fmax: (ncell).  Units after
 * INIT.f90:611-631 (mm^3/mm^3, mm/s, -, mm). */
int h9g_set_params(h9g_ctx *ctx, const float *theta_s, const float *hksat,
                   const float *bsw, const float *psi_s, const float *fmax);
/* Initial state of INIT.f90:707-811 for every cell (smp = 0). */
int h9g_init_state(h9g_ctx *ctx);
/* Packed per-cell state, fields in this order, each (width, ncell) with
 * width-fastest:  h2osoi_liq(L) h2osoi_liq_ma(L) smp(L) rootr_col(L+1)
 * zwt wa LAI LAI_litter plant_mass plant_foliage_mass plant_length rdepth
 * -> h9g_state_size(L) = 4L+9 floats per cell.  (The device keeps these as
 * rows of ncell: hybrid9_amd/csrc/h9g_rows.h describes that layout, once.) */
int h9g_state_size(int nlayers);
int h9g_set_state(h9g_ctx *ctx, const float *packed);
int h9g_get_state(h9g_ctx *ctx, float *packed);

/* --- forcing (READ_PGF.f90) ------------------------------------------ */
/* Copies nday days of forcing, 7 arrays of (ncell, nday) stacked as
 * (7, nday, ncell), into slot `slot`.  async=1 enqueues the copy on the
 * context's copy stream (host memory should be pinned, see
 * h9g_host_alloc); h9g_run_year orders itself after it. */
int h9g_push_forcing(h9g_ctx *ctx, int slot, int nday, const float *forcing,
                     int async);
/* Same from device memory (e.g. a slab already resident in HBM). */
int h9g_push_forcing_device(h9g_ctx *ctx, int slot, int nday,
                            const float *dev_forcing);
/* Device pointer of a slot (capacity max_days), for zero-copy producers. */
float *h9g_forcing_slot(h9g_ctx *ctx, int slot);
void *h9g_host_alloc(size_t bytes);   /* pinned host memory */
void h9g_host_free(void *p);

/* --- the hot path ----------------------------------------------------- */
/* Advance every cell through calendar year `jyear` (365/366 days by
 * INIT.f90:844-859) using the forcing in `slot` starting at its day 0.
 * Enqueued on the compute stream; returns after launch.  Errors are
 * reported by the next h9g_sync. */
int h9g_run_year(h9g_ctx *ctx, int slot, int jyear);
/* Wait for all work; returns the first STOP code raised, if any. */
int h9g_sync(h9g_ctx *ctx);
int h9g_last_error(h9g_ctx *ctx, h9g_error *err);
/* Every cell's STOP record since the state was last set: rec is 4 rows of
 * ncell int32 -- H9G_ERR_* code (0: none), 0-based day, substep, and the
 * bits of the float value the reference prints (failed cells stop; their
 * annual means are NaN). */
int h9g_get_errors(h9g_ctx *ctx, int32_t *rec);

/* --- the reference's own cell order (HYBRID9.f90:93-130) ---------------- */
/* Advances every cell through years jyear0 .. jyear0+nyears-1 (the forcing
 * of year jyear0+k in slots[k]) as ONE pass of the reference's decade loop
 * runs them on one rank (or on every rank of h9g_set_chains): the cell
 * loop (:120-295) visits the land cells in context order, and HYDROLOGY's
 * module array smp (SHARED.f90:198) is not per cell, so a land cell's
 * first substep reads in beta (HYDROLOGY.f90:270-275) the smp its
 * predecessor left behind; the first land cell reads what the last one
 * holds when the call starts (at a fresh start all smp are 0; the
 * reference leaves smp uninitialised, INIT.f90:109).  Call it once per
 * decade of the reference (1901-1910, 1911-1920, ...) with the rank's
 * cells in (y, x) order to reproduce the reference run bit for bit.
 * h9g_run_year's isolated-cell semantics (every cell its own smp) differ
 * from this by up to 4e-2 relative from the second decade on (DESIGN.md
 * §2).  Solved on the device: each pass re-runs the decade for the cells
 * whose input smp changed, until none does; a re-run cell leaves the pass
 * at the first year end where its state equals its previous run's (its
 * later years are then unchanged, bit for bit).  annual: (nyears, 12+L,
 * ncell) host (may be NULL); passes (may be NULL): decade passes run.
 * Synchronous; returns 0 or the STOP code of the first failing cell in
 * context order (h9g_last_error, with its year). */
int h9g_run_decade_ordered(h9g_ctx *ctx, const int32_t *slots, int jyear0,
                           int nyears, float *annual, int32_t *passes);
/* The reference's decade loop over several decades: years jyear0 ..
 * jyear0+nyears-1 (the forcing of year jyear0+k in slots[k], every year's
 * slot resident for the whole call) cut into the reference's decades
 * (1901-1910, 1911-1920, ...), each run as h9g_run_decade_ordered runs
 * one, with the same results bit for bit.  The years' slots must be
 * distinct (H9G_EINVAL otherwise).  The decades overlap on the
 * device: a decade's first pass starts as soon as the previous decade's
 * first pass and year-1 re-run are done, and that decade's remaining
 * re-runs ride in its year launches.  annual: (nyears,
 * 12+L, ncell) host (may be NULL); passes (may be NULL): one int32 per
 * decade.  A cell that STOPs leaves the later decades' chains (the
 * reference would end the program there; h9g_last_error reports the first
 * STOP in decade then context order).  Synchronous. */
int h9g_run_ordered(h9g_ctx *ctx, const int32_t *slots, int jyear0, int nyears,
                    float *annual, int32_t *passes);
/* Splits the context's cells into independent chains for
 * h9g_run_decade_ordered, one per reference MPI rank: chain[c] (ncell
 * int32, 0 <= id < ncell) is the rank whose block holds cell c (INIT.f90:
 * 271-274, 427-444; hybrid9_amd.shard.reference_blocks).  Each chain runs
 * its cells in context order, as that rank runs its block, so a context
 * holding several ranks' blocks reproduces them all at once.  NULL: one
 * chain (the default, a one-rank run). */
int h9g_set_chains(h9g_ctx *ctx, const int32_t *chain);
/* Work of the last h9g_run_decade_ordered: out[0..n) of passes, cells
 * re-run (summed over the passes), cell-years re-run, and year launches of
 * the re-runs (a re-run cell leaves at the first year end where its state
 * is its previous run's again), then the cells of each re-run launch in
 * order.  Returns the count written (<= 4 + launches). */
int h9g_decade_stats(h9g_ctx *ctx, int64_t *out, int n);
/* How the last ordered call overlapped its decades: out[0..n) of decades,
 * year launches of the first passes, re-run years that rode in them and
 * their cell-years, re-run years launched alone and their cell-years, cells
 * left out of a first pass (still re-running the decade before), cells the
 * checks' day-1 probe ran and those of them it kept for a re-run, then each
 * decade's passes.  Returns the count written. */
int h9g_ordered_stats(h9g_ctx *ctx, int64_t *out, int n);

/* --- LCLIM single-site path (HYBRID9.f90:339-480) ---------------------- */
/* Runs nday days of the site path for every cell of the context: per
 * substep forcing, a day-of-year LAI schedule, HYDROLOGY only (no GROW).
 * Replaces the LCLIM branch :339-480 (its CSV reads :353-439 are done by
 * the caller, e.g. hybrid9_amd.site.read_lclim).  Host arrays, [row][cell]:
 *   sub   (nday*nisurf, 5, ncell): tak (degC), rh (%), Rnet (W m-2),
 *         PAR, ppt (mm per substep)        -- LCLIM_array2 (22,25,14,16,35)
 *   daily (nday, 2, ncell): huss (kg/kg), ps (Pa)   -- LCLIM_array (5,6)
 *   lai   (nday, 3, ncell): (LAI, a, b): LAI = LAI, then
 *         LAI_litter = LAI_litter + a - b; NaN leaves a value unchanged
 *         (encodes the schedule of :380-417)
 *   diag  (nday, 11, ncell) out: evap_day, evap_grnd_day, theta(1:4),
 *         theta_ma(1), LAI, LAI_litter, w_i, fT (the daily line :464-469;
 *         w_i = fT = 0 as GROW does not run; NaN for masked/failed cells)
 * Synchronous.  Updates the state (h2osoi_liq, smp, zwt, wa, LAI,
 * LAI_litter).  Returns 0 or a STOP code (h9g_last_error: day counts
 * from the start of the run, year = 0). */
int h9g_run_site(h9g_ctx *ctx, int nday, const float *sub, const float *daily,
                 const float *lai, float *diag);

/* --- daily diagnostics of a focus window (HYBRID9.f90:221-229) ---------- */
/* The line the reference writes to LCLIM/daily_diag.csv each day when
 * INTERACTIVE is set: evap_day, evap_grnd_day, theta(1:4), theta_ma(1), LAI,
 * LAI_litter, w_i, fT (jyear and DOY are the caller's).  The year kernels
 * store nothing per day; the selected cells are run a second time by a small
 * shadow kernel from the same start state and forcing, which follows the
 * year kernel's trajectory bit for bit.  It only reads: state,
 * annual means and STOP records are the same with or without a selection.
 * A cell that STOPs has NaN from the STOP day on; a masked cell, or one that
 * had stopped before the run, on every day.  With grow_on = 0, w_i = fT = 0. */
#define H9G_NDAILY 11
/* Selects the cells whose daily line later runs record: cells[0..nsel) are
 * context indices, strictly increasing.  nsel = 0 turns it off (the
 * default).  H9G_EINVAL for a bad list, H9G_ENOMEM if the buffers do not
 * fit.  h9g_run_year then launches the shadow run on the compute stream
 * before its year kernel; h9g_run_decade_ordered replays the selected cells
 * over the decade once its fixed point has settled, each from its decade
 * start with the smp its predecessor in the chain hands it; h9g_run_ordered
 * then runs its decades one after another (no overlap; the same results bit
 * for bit, h9g_ordered_stats reports the last decade only).  The lines take
 * nyears x max_days x 11 x nsel floats of device memory, allocated by the
 * run and released with the context (not part of h9g_config_bytes). */
int h9g_set_daily(h9g_ctx *ctx, int nsel, const int32_t *cells);
/* Daily lines of year k (0-based) of the last h9g_run_year (k = 0),
 * h9g_run_decade_ordered or h9g_run_ordered call: out (nday_k, 11, nsel),
 * selection order.  Synchronises.  H9G_ESTATE if nothing was recorded,
 * H9G_EINVAL for a bad k. */
int h9g_get_daily(h9g_ctx *ctx, int k, float *out);

/* --- monthly output: month-end running sums from the year kernels ------- */
/* The reference writes one mean per cell and year.  With monthly recording
 * on, every year kernel also stores, at the end of each calendar month's
 * last day (INIT.f90:844-859: day 31, 59, 90, ... 365, one later from
 * February on in a year of 366 days), the year's 12+L running sums as they
 * then stand: after GROW and the additions of HYBRID9.f90:235-254,
 * undivided, in h9g_get_annual's row order --
 *   npp_sum plant_mass_sum rnf_sum 0 tas..rhs sums theta_sum(1..L)
 *   h2osoi_sum_total
 * (row evap is the reference's zero: it never accumulates evap_sum).  The
 * sums are never reset, so the annual means stay the reference's; snapshot
 * 11 is the year's final sums, and divided as :263-290 divides them it gives
 * the annual means bit for bit.  A snapshot is a prefix of the reference's
 * own f32 summation.  The mean of month m is derived on the host from two
 * snapshots, in double: (S[m] - S[m-1]) / days_m  (S[-1] = 0; divisor
 * days_m * nisurf for rnf, 1 for npp, a monthly total): deterministic, but
 * derived from f32 running sums, not a reference quantity.
 * A cell that reaches a reference STOP in a year has NaN in all twelve
 * months of that year and of every later one; a masked cell, or one that
 * had stopped before the run, throughout.
 * Monthly kernels are the year kernels under other names; with recording off
 * (the default) not one launch, allocation or synchronisation is added, and
 * annual means, state, STOP records and daily lines are the same bit for bit
 * either way.  The snapshots take nyears x 12 x (12+L) x ncell floats of
 * device memory per call (1.3 GB for 20 years of the 0.5 deg grid), allocated
 * by the run and released with the context (not part of h9g_config_bytes);
 * H9G_ENOMEM if it does not fit. */
#define H9G_NMONTHS 12
int h9g_set_monthly(h9g_ctx *ctx, int on);
/* Snapshots of year k (0-based) of the last h9g_run_year (k = 0),
 * h9g_run_decade_ordered or h9g_run_ordered call: out (12, 12+L, ncell),
 * cell fastest.  Synchronises.  H9G_ESTATE if nothing was recorded,
 * H9G_EINVAL for a bad k. */
int h9g_get_monthly(h9g_ctx *ctx, int k, float *out);

/* --- evapotranspiration output: the ET year kernels ---------------------- */
/* The reference sets evap_sum = 0 at the start of a year (HYBRID9.f90:137)
 * and never adds to it, so row evap of the annual means and of every
 * snapshot is +0.  With ET recording on, every year launch of the context
 * (the cell order's day-1 probes included) runs the ET year kernels, the
 * year kernels under other names, which accumulate, in f32 with no
 * contraction,
 *   evap_sum = evap_sum + (qflx_evap_grnd + qflx_tran_veg_col) * dt
 * after every substep -- the expression of :207-208's evap_day in the form
 * of rnf_sum's HYDROLOGY.f90:1282-1283, qflx_evap_grnd after the
 * MIN(em1, .) of :396-400, dt = 86400 / NISURF -- and survive the exact
 * re-run.  Row evap of h9g_get_annual is then evap_sum / FLOAT(nt * NISURF)
 * as :276 is written: the convention of row rnf (the sum is in mm, the mean
 * mm per substep; the file attribute "mm/s" is the reference's label and
 * stays).  Row evap of a month-end snapshot is evap_sum as it stands, like
 * rnf_sum.  Only the total is recorded: the ground/canopy partition stays
 * with the daily line.  Every other annual and monthly row, the state, the
 * STOP records and the daily lines are the same bits with recording on or
 * off; a cell that stops has NaN in row evap like in every other.  With
 * recording off (the default) nothing changes: no launch, allocation or
 * synchronisation is added, and row evap is the reference's +0.  No buffer
 * of its own (h9g_config_bytes is unchanged).  H9G_EINVAL for a null
 * context.  h9g_kernel_name then reports the ET kernel. */
int h9g_set_evap(h9g_ctx *ctx, int on);

/* --- day records: day-end records of every cell from the year kernels ---- */
/* The daily line above is a shadow run of selected cells.  With day
 * recording on, every year kernel stores H9G_NDAYREC floats for every cell
 * and every day d = 0 .. nt-1 of the year, taken after the day's last
 * substep, after GROW and after the additions of HYBRID9.f90:235-254 (where
 * the month-end snapshots are taken):
 *   row 0  rnf_sum: the year's running runoff sum as it stands (mm)
 *   row 1  evap_sum: the year's running ET sum as it stands (mm; the ET
 *          section's sum)
 *   row 2  W = h2osoi_liq(1) + ... + h2osoi_liq(L), f32, added in that
 *          order (mm)
 *   row 3  theta(1) of HYDROLOGY.f90:1233, the day's addend to theta_sum(1)
 *   row 4  zwt (mm)
 *   row 5  wa (mm)
 *   row 6  LAI after the day's GROW
 * Rows 0 and 1 are cumulative, like the month-end snapshots and for the same
 * reason: nothing is reset, every record is a prefix of the reference's own
 * f32 summation and the year's sums stay the reference's.  The day's runoff
 * and ET are derived on the host, in double: (double)S[d] - (double)S[d-1]
 * with S[-1] = 0, in mm per day: deterministic, but derived, not reference
 * quantities.  Row 0 and row 1 of a year's last day, divided by
 * FLOAT(nt * NISURF), are rows rnf and evap of the annual means; at a month's
 * last day they are rows rnf and evap of that month's snapshot.
 * Day recording needs the ET sum, so it rides on ET recording:
 * h9g_set_days(ctx, 1) returns H9G_ESTATE unless h9g_set_evap is on, and
 * h9g_set_evap(ctx, 0) returns H9G_ESTATE while day recording is on.
 * A cell that reaches a reference STOP on day e of a year keeps its records
 * of days 0 .. e-1 of that year and has NaN from day e on and in every later
 * year (the daily line's convention: the reference ends before the day
 * completes); a masked cell, or one that had stopped before the year, has NaN
 * throughout.
 * The day kernels are the ET year kernels under other names
 * (h9g_kernel_name reports them); with recording off (the default) not one
 * launch, allocation or synchronisation is added, and with it on annual
 * means, month-end snapshots, state, STOP records and daily lines are the
 * bits of an ET run without it.  h9g_spinup records nothing: H9G_ESTATE with
 * day recording on.  The records take max_days x 7 x ncell floats of device
 * memory for a year in cell order and as much again in slot order (0.7 GB
 * each for the 0.5 deg grid); an ordered call retains nyears x max_days x 7 x
 * ncell floats and holds as much per decade in flight (the day rows live
 * beside that year's annual rows, and the same launches write them: first
 * passes, list re-runs, re-runs riding as a second group; the decades stay
 * overlapped).  All of it is allocated by the run and released with the
 * context (not part of h9g_config_bytes); H9G_ENOMEM if it does not fit.
 * Day recording combines with monthly recording and with a daily selection
 * wherever those two combine. */
#define H9G_NDAYREC 7
int h9g_set_days(h9g_ctx *ctx, int on);
/* Day records of year k (0-based) of the last h9g_run_year (k = 0),
 * h9g_run_decade_ordered or h9g_run_ordered call: out (nday_k, 7, ncell),
 * cell fastest.  Synchronises.  H9G_ESTATE if nothing
 * was recorded, H9G_EINVAL for a bad k. */
int h9g_get_days(h9g_ctx *ctx, int k, float *out);

/* --- day statistics: per-cell annual indices from the day records --------- */
/* The day records are the only output finer than a month, and a year of them
 * is max_days x 7 x ncell floats.  h9g_get_daystats reduces them on the
 * device, over the day axis, where they lie: per cell and year H9G_NDAYSTAT
 * numbers, out (nk, 17, ncell) doubles, cell fastest, for years k0 ..
 * k0+nk-1 of what the last h9g_run_year (k0 = 0, nk = 1),
 * h9g_run_decade_ordered or h9g_run_ordered call recorded.  Synchronises, as
 * h9g_get_days does.  H9G_ESTATE if nothing was recorded; H9G_EINVAL for a bad
 * span, a null pointer, a NaN threshold or a non-zero `reserved`.
 *
 * R[d][r] is the year's record (f32), d = 0 .. nt-1; S[d] = (double)R[d][0]
 * with S[-1] = 0, and the same for row 1.  Each of
 *   q[d]  = S[d] - S[d-1]     the day's runoff (h9g_write_dxy_nc's difference,
 *                             before its rounding to f32), mm
 *   e[d]  = the same from row 1, mm
 *   q7[d] = S[d] - S[d-7]     for d = 6 .. nt-1, with S[-1] = 0 at d = 6, mm
 * is one IEEE operation.  A candidate that is NaN is skipped (a STOP day and
 * later, a masked cell); a day is valid when none of its seven values is NaN.
 *   row 0      ndays                  valid days
 *   row 1, 2   q_max, q_max_day       largest q[d]; 0-based day of its first occurrence
 *   row 3      q7_min                 smallest q7[d]
 *   row 4      q_days                 days with q[d] >= (double)q_thr
 *   row 5      e_max                  largest e[d]
 *   row 6, 7   w_min, w_min_day       smallest row 2; first day
 *   row 8      w_max                  largest row 2
 *   row 9      theta1_min             smallest row 3
 *   row 10     dry_days               days with row 3 < theta_thr
 *   row 11     dry_spell              longest run of consecutive dry days; a day that
 *                                     is not dry, or is NaN, ends a run
 *   row 12     zwt_min                smallest row 4 (shallowest table)
 *   row 13     wet_days               days with row 4 <= zwt_thr
 *   row 14, 15 lai_max, lai_max_day   largest row 6; first day
 *   row 16     green_days             days with row 6 >= lai_thr
 * Extremes are kept by a strict comparison in day order: a later equal value
 * never replaces an earlier one, and the first candidate that is not NaN
 * starts the extreme.  With no candidate an extreme is NaN, its day -1 and the
 * counts 0.  Counts and day numbers are exact in a double.  There is no
 * floating-point sum whose order matters: every row is exact and comparable
 * bit for bit with a restatement in numpy (hybrid9_amd.day_stats).
 * Nothing here is a reference quantity: like the days' amounts and the monthly
 * means it is deterministic and derived from the reference's f32 running sums.
 * One memory-bound kernel (h9g_daystat_kernel) reads the records where
 * h9g_get_days reads them and never copies them; no year kernel and no run
 * path changes.  Its only allocation is the nk x 17 x ncell doubles of the
 * result, made by the first call, grown when needed and released with the
 * context (not part of h9g_config_bytes).  Without a call nothing is added
 * anywhere: no launch, allocation or synchronisation. */
#define H9G_NDAYSTAT 17
typedef struct {
  float q_thr;      /* mm/day:   a "runoff day" has q[d] >= q_thr (compared in double) */
  float theta_thr;  /* mm3/mm3:  a "dry day" has theta1[d] < theta_thr (f32 compare)  */
  float zwt_thr;    /* mm:       a "wet day" has zwt[d] <= zwt_thr                    */
  float lai_thr;    /*           a "green day" has LAI[d] >= lai_thr                  */
  int32_t reserved[4];  /* 0 */
} h9g_daystat_opts;
int h9g_get_daystats(h9g_ctx *ctx, int k0, int nk, const h9g_daystat_opts *opts, double *out);

/* --- day quantiles: order statistics of a daily series from the day records */
/* The day statistics are streaming reductions, one year at a time.  An order
 * statistic of a cell's daily series -- the flow-duration curve, the median
 * water table, a low percentile of top-layer moisture -- is not: it needs a
 * selection, and it may pool several years.  h9g_get_dayquant selects on the
 * device, from the day records where they lie, for years k0 .. k0+nk-1 of what
 * the last h9g_run_year (k0 = 0, nk = 1), h9g_run_decade_ordered or
 * h9g_run_ordered call recorded.  Synchronises, as h9g_get_days does.
 * H9G_ESTATE if nothing was recorded; H9G_EINVAL for a bad span (a pooled span
 * holds at most 512 years), a null pointer, `series` outside 0..6, `nq`
 * outside 1..H9G_NQUANT_MAX, a `p` outside [0, 1] or NaN, `pooled` not 0 or 1,
 * or a non-zero `reserved`.
 *
 * Candidates.  Series 0 and 1: q[d] and e[d] exactly as h9g_get_daystats
 * defines them, one IEEE subtraction of the widened f32 running sums with
 * S[-1] = 0 at every year's day 0 (in a pooled span every year restarts).
 * Series 2..6: the f32 value of record row 2..6 widened to double.  A NaN
 * candidate is skipped (a STOP day and later, a masked cell); m is the number
 * of candidates left, per year, or over all years of the span when pooled.
 * Order.  The total order on the doubles' bits: the sign-magnitude pattern
 * mapped to a monotone unsigned key, so -0 sorts before +0 and equal values
 * are interchangeable: x_(0) <= ... <= x_(m-1).
 * Result.  out (nres, 1 + 2 nq, ncell) doubles, cell fastest, nres = pooled ?
 * 1 : nk.  Row 0 is m.  For p[i], g = p[i] * (double)(m - 1) (one IEEE
 * multiply) and j = floor(g): row 1 + 2i is x_(j), row 2 + 2i is
 * x_(min(j + 1, m - 1)); with m = 0 both are NaN.  A cell that STOPs on day e
 * contributes its days before e; a masked cell has m = 0.  Nothing is
 * interpolated on the device and there is no floating-point sum anywhere:
 * every row is exact and comparable bit for bit with a restatement in numpy
 * (hybrid9_amd.day_order_stats).  The host derives the quantile, lo + (hi -
 * lo) * (g - j) in double (lo itself where lo and hi are equal or g is whole,
 * so an infinite value stays one): deterministic and derived, like the
 * monthly means.  Hydrology counts from the top: its "Q95", the flow exceeded
 * 95 % of the time, is p = 0.05 here, and "Q5" is p = 0.95.
 * One kernel (h9g_dayquant_kernel) selects all nq ranks by the key's digits,
 * most significant first, streaming the series once per digit and once more
 * for the upper neighbours; it reads the records where h9g_get_days reads
 * them and never copies them; no year kernel and no run path changes.  Its
 * only allocation is the result, made by the first call, grown when needed
 * and released with the context (not part of h9g_config_bytes); its working
 * state lives in registers and LDS.  Without a call nothing is added
 * anywhere: no launch, allocation or synchronisation. */
#define H9G_NQUANT_MAX 16
typedef struct {
  int32_t series;      /* 0: q  1: e  2..6: record rows 2..6 (W, theta1, zwt, wa, LAI) */
  int32_t nq;          /* 1 .. H9G_NQUANT_MAX */
  int32_t pooled;      /* 0: one result per year of the span; 1: one for the whole span */
  int32_t reserved;    /* 0 */
  double p[H9G_NQUANT_MAX];   /* each in [0, 1], not NaN; any order, repeats allowed */
} h9g_dayquant_opts;
int h9g_get_dayquant(h9g_ctx *ctx, int k0, int nk, const h9g_dayquant_opts *opts, double *out);

/* --- spin-up to equilibrium: cycle a forcing period, retire settled cells - */
/* The model cold-starts from INIT.f90:707-811, and the reference's only
 * answer is to repeat years (its LCLIM loop re-reads the site years
 * NYR_SPIN_UP times).  h9g_spinup repeats a forcing period on the device
 * until the cells stop changing, tests every cell on its own, and with
 * freeze = 1 launches only the cells that have not settled yet.
 *
 * A cycle runs years jyear0 .. jyear0+nyears-1 as h9g_run_year runs them
 * (isolated cells: every cell its own smp), the forcing of year jyear0+k in
 * slots[k]; every cycle the same calendar years.  The slots are distinct and
 * stay resident for the whole call (H9G_EINVAL otherwise, as
 * h9g_run_ordered).
 *
 * After cycle k = 1, 2, ... every cell that ran it is tested against its own
 * state one cycle earlier (cycle 0: the state the call found).  In double,
 * from the f32 state, one IEEE operation per step:
 *   W   = h2osoi_liq(1) + ... + h2osoi_liq(L), added in that order, then + wa
 *   d_w = |W_k - W_{k-1}|                                   (mm)
 *   d_z = |zwt_k - zwt_{k-1}|                               (mm)
 *   d_p = 0 if pm_k == pm_{k-1}, else |pm_k - pm_{k-1}| / |pm_{k-1}|
 *         (plant_mass; +inf from a zero pm_{k-1})
 * The cell settles at cycle k when k >= min_cycles, d_w <= tol_water,
 * d_z <= tol_zwt and d_p <= tol_plant; a NaN drift never settles.  A
 * tolerance of +inf turns its criterion off, 0 demands a bit-exact fixed
 * point of that quantity.  H9G_EINVAL for a negative or NaN tolerance,
 * max_cycles < 1, min_cycles < 1 or > max_cycles, freeze not 0 or 1, or
 * reserved not 0.
 *
 * freeze = 1: a settled cell keeps the state, annual means and STOP record
 * its last cycle left and is not launched again; the later cycles are list
 * launches of the cells still active (cells in increasing order; the kernel
 * by the list's length, as the cell order's re-runs).  Cells are independent,
 * so every other cell's bits are what they would be with it running.  The
 * call ends after the first cycle that leaves no active cell, or after
 * max_cycles.
 * freeze = 0: every cycle is an every-cell launch, cell_cycle records the
 * first cycle at which the cell met the criterion, and the call ends after
 * the first cycle in which every tested cell meets it, or after max_cycles;
 * the end state is that of cycles_run x nyears h9g_run_year calls, bit for
 * bit.
 *
 * A cell that reaches a reference STOP in a cycle leaves the run (the year
 * kernels skip it); the others go on.  A masked cell, or one that had stopped
 * before the call, never runs.  Returns 0, or the code of the first STOP in
 * context order, as h9g_sync (h9g_last_error: that cell's record, with the
 * year of the cycle it stopped in).
 *   cycles_run    cycles run (may be NULL)
 *   cell_cycle[c] (ncell, may be NULL)  k > 0: settled at cycle k; 0: still
 *                 active when the call ended; -1: masked or stopped before the
 *                 call; -2: stopped during the call
 *   history       (max_cycles, H9G_NSPIN), may be NULL; row k-1 of cycle k:
 *                 cells run, cells settled at k (freeze = 0: that met the
 *                 criterion for the first time), cells stopped in k, then the
 *                 maxima of d_w, d_z and d_p over the cells tested in k (0
 *                 with none; a NaN drift is not counted).  Rows of cycles not
 *                 run are 0.
 * After the call h9g_get_state holds every cell's state after the last cycle
 * it ran, h9g_get_annual the means of the last year of that cycle, and
 * h9g_get_diagnostics is recomputed once over exactly those rows;
 * h9g_launch_stats counts the launches as usual.
 * Spin-up records nothing: H9G_ESTATE with a daily selection or monthly
 * recording on.  ET recording (h9g_set_evap) is allowed.  Synchronous.  One
 * small kernel (h9g_spin_kernel) and one read of eight doubles per cycle;
 * three doubles and three int32 per cell of device memory, allocated by the
 * first call and released with the context (not part of h9g_config_bytes).
 * Without a call nothing is added anywhere: no launch, allocation or
 * synchronisation. */
typedef struct {
  int32_t max_cycles;   /* >= 1 */
  int32_t min_cycles;   /* >= 1: no cell settles before this cycle */
  int32_t freeze;       /* 1: a settled cell leaves the later cycles; 0: every cell runs every cycle */
  int32_t reserved;     /* 0 */
  double tol_water;     /* mm: |W_k - W_{k-1}|, W = sum_i h2osoi_liq(i) + wa */
  double tol_zwt;       /* mm: |zwt_k - zwt_{k-1}| */
  double tol_plant;     /* relative: |pm_k - pm_{k-1}| / |pm_{k-1}| (plant_mass) */
} h9g_spinup_opts;
#define H9G_NSPIN 6
int h9g_spinup(h9g_ctx *ctx, const int32_t *slots, int jyear0, int nyears,
               const h9g_spinup_opts *opts, int32_t *cycles_run,
               int32_t *cell_cycle /* ncell, may be NULL */,
               double *history /* max_cycles x H9G_NSPIN, may be NULL */);

/* --- outputs (HYBRID9.f90:263-290) ------------------------------------ */
/* Annual means of the last year run, (12+L) rows of (ncell):
 * npp plant_mass rnf evap tas rlds rsds huss ps pr rhs theta(1..L)
 * theta_total  (axy_* of SHARED.f90:478-493, NaN for failed cells). */
int h9g_get_annual(h9g_ctx *ctx, float *annual);
/* Global diagnostics of the last year (FP64 sums over this context's
 * cells, deterministic order): see H9G_DIAG_* in DESIGN.md.  Intended
 * for an all-reduce across GPUs.  dev_out (may be NULL) receives a
 * device-side copy; host_out (may be NULL) a host copy. */
int h9g_get_diagnostics(h9g_ctx *ctx, double *host_out, double *dev_out);
/* Stream-ordered variant, no host synchronisation: copies the diagnostics
 * into device buffer dev_out after the work already queued on `stream` (a
 * hipStream_t, NULL = legacy default stream), and makes `stream` wait for
 * the copy -- e.g. the stream an RCCL all-reduce of dev_out runs on. */
int h9g_get_diagnostics_async(h9g_ctx *ctx, double *dev_out, void *stream);

/* --- synthetic inputs (hybrid9_amd/synth.py, bit-identical) ----------- */
/* Cells are identified by their grid id (iy*nx+ix) and latitude. */
int h9g_set_cells(h9g_ctx *ctx, const int64_t *gid, const float *lat);
/* The synthetic land mask (host): the nland grid ids of an nx x ny grid,
 * raster order, and their latitudes (synth.land_cells / cell_lat). */
int h9g_land_cells(int nx, int ny, int nland, uint64_t seed, int64_t *gid,
                   float *lat);
int h9g_synth_params(h9g_ctx *ctx, uint64_t seed);
int h9g_synth_forcing(h9g_ctx *ctx, int slot, uint64_t seed, int day0,
                      int nday);

/* --- NetCDF I/O (hybrid9_amd/csrc/h9g_io.cpp): reads netCDF-4 (HDF5,
 * through the image's libhdf5, loaded on first use) and classic CDF-1/2;
 * writes CDF-2 ------------------------------------------------------------ */
/* WRITE_NET_CDF_3DR.f90:93-263: annual means (h9g_get_annual layout, 12+L
 * rows of ncell) of the cells gid (grid ids iy*nx+ix, row iy from the
 * north) to axyYYYY.nc with the reference's dimensions, variable names,
 * units and NaN _FillValue; zc = layer centre depths (L).  Host only. */
int h9g_write_axy_nc(const char *path, int nx, int ny, int nlayers,
                     const float *zc, int ncell, const int64_t *gid,
                     const float *annual);
/* mxyYYYY.nc: the monthly means of year jyear derived from its month-end
 * snapshots (h9g_get_monthly, (12, 12+L, ncell)) as described there, with
 * axyYYYY.nc's variables, names, units and NaN fill under a leading
 * dimension `month` of 12; net primary production in g[DM]/m^2/month.
 * CDF-2.  Host only. */
int h9g_write_mxy_nc(const char *path, int nx, int ny, int nlayers,
                     const float *zc, int ncell, const int64_t *gid, int jyear,
                     int nisurf, const float *snapshots);
/* The same file from the snapshots of an ET run (h9g_set_evap): row
 * evaporation is divided by days_m * nisurf, like runoff. */
int h9g_write_mxy_nc_evap(const char *path, int nx, int ny, int nlayers,
                          const float *zc, int ncell, const int64_t *gid,
                          int jyear, int nisurf, const float *snapshots);
/* dxyYYYY.nc: one year of day records (h9g_get_days, (nday, 7, ncell)) of
 * the cells gid under a leading dimension `time` of nday, with axyYYYY.nc's
 * latitude / longitude schema and NaN _FillValue: runoff and
 * evapotranspiration (mm/day: the day's amounts, derived from the running
 * sums in double as described there), soil_water (mm), soil_water_top_layer
 * (mm^3/mm^3), water_table_depth (mm), aquifer_water (mm) and LAI.  CDF-2,
 * written variable by variable.  Host only. */
int h9g_write_dxy_nc(const char *path, int nx, int ny, int nlayers,
                     const float *zc, int ncell, const int64_t *gid, int jyear,
                     int nday, const float *records);
/* sxyYYYY.nc: one year of day statistics (h9g_get_daystats, (17, ncell)
 * doubles) of the cells gid as 17 float64 variables on axyYYYY.nc's latitude /
 * longitude grid, named as the rows above, NaN _FillValue, units as
 * attributes (counts in "days", day numbers in "day of year (0-based)"); the
 * four thresholds and the year are global attributes.  CDF-2.  Host only. */
int h9g_write_sxy_nc(const char *path, int nx, int ny, int ncell, const int64_t *gid, int jyear,
                     const h9g_daystat_opts *opts, const double *stats);
/* qxyYYYY.nc (qxyYYYY_YYYY.nc for a pooled span): one result of
 * h9g_get_dayquant, quant (1 + 2 nq, ncell) doubles, of the cells gid on
 * axyYYYY.nc's latitude / longitude grid: dimension `quantile` (nq) with the
 * coordinate variable p, then count(latitude, longitude) (row 0) and lower,
 * upper and value(quantile, latitude, longitude) -- the two order statistics
 * and the quantile interpolated between them as described there -- all
 * float64 with NaN _FillValue.  The series' name (q, e, soil_water, theta1,
 * zwt, wa, LAI), year_first, year_last and pooled are global attributes.
 * CDF-2.  Host only. */
int h9g_write_qxy_nc(const char *path, int nx, int ny, int ncell, const int64_t *gid,
                     int year_first, int year_last, const h9g_dayquant_opts *opts, const double *quant);
/* READ_PGF.f90 / READ_NET_CDF_3DR.f90: days [t0, t0+nt) of variable 4
 * (time, lat, lon) of the 7 PGF files (tas rlds rsds huss ps pr rhs)
 * gathered at the grid ids gid into out (7, nt, ncell).  Host only. */
int h9g_nc_forcing_read(const char *const *paths, int nx, int ny, int ncell,
                        const int64_t *gid, int t0, int nt, float *out);
/* NTIMES of a PGF file: length of its 'time' dimension. */
int h9g_nc_ntimes(const char *path);
/* Stage profile of the last completed forcing read (any thread, any
 * context): out[0..n) of, in order, wall s, serial setup s (headers and
 * chunk tables), pool threads, jobs, then thread-seconds summed over the
 * pool of pread, inflate + unshuffle, gather, and other layouts (classic
 * rows / H5Dread), then stored bytes read, bytes decoded, values gathered
 * and the pool's wall s.  Returns the count written (<= H9G_IO_NSTATS). */
#define H9G_IO_NSTATS 12
int h9g_nc_read_stats(double *out, int n);
/* The same read on a host thread into pinned memory, then an async copy
 * into `slot` (needs h9g_set_cells); h9g_run_year on the slot waits. */
int h9g_nc_forcing_prefetch(h9g_ctx *ctx, int slot, const char *const *paths,
                            int nx, int ny, int t0, int nt);

/* --- soil parameter build (INIT.f90:492-680) --------------------------- */
/* One soil layer (0-based) of the context's cells (h9g_set_cells): the
 * 60x60 block average of the layer's 30" fields theta_s (0.001 cm3/cm3),
 * k_s (cm/day), lambda (0.001), psi_s (cm) over pixels with theta_s >= 0,
 * and the unit conversions of INIT.f90:611-628.  Fields: (ny*60) rows of
 * nx*60 floats, row 0 north; device pointers if on_device, else host. */
int h9g_soil_layer(h9g_ctx *ctx, int layer, const float *ts, const float *ks,
                   const float *lm, const float *ps, int nx, int ny,
                   int on_device);
/* INIT.f90:661-680 once all layers are built: Fmax of the soiled cells
 * from the 0.5 deg integer grids soil_tex and fmax (ny, nx); completes the
 * parameters (replaces h9g_set_params). */
int h9g_soil_fmax(h9g_ctx *ctx, const int32_t *soil_tex, const int32_t *fmax,
                  int nx, int ny);
/* Device ms of the last soil layer's block-average kernel; number of its
 * cells summed in the reference's sequential order (non-integer data). */
float h9g_last_soil_ms(h9g_ctx *ctx);
int h9g_last_soil_slow(h9g_ctx *ctx);
/* Parameters back to the host, h9g_set_params layouts. */
int h9g_get_params(h9g_ctx *ctx, float *theta_s, float *hksat, float *bsw,
                   float *psi_s, float *fmax);

/* --- measurement ------------------------------------------------------ */
/* Device time (HIP events on the compute stream) of the last year kernel,
 * and of all year kernels since the last reset. */
float h9g_last_kernel_ms(h9g_ctx *ctx);
double h9g_total_kernel_ms(h9g_ctx *ctx, int reset);
const char *h9g_kernel_name(h9g_ctx *ctx);
/* Per kernel kind 1..6 (pair, solo, solo+pair, pair2, pair11, pair1 -- the
 * one-column kernel of short re-run lists), 3 doubles each: year launches,
 * cell-years and device ms since the last reset (synchronises); then row 7,
 * the cell order's one-day probe launches (launches, cells, ms).  Returns
 * the count written (<= 21). */
int h9g_launch_stats(h9g_ctx *ctx, double *out, int n, int reset);
/* Device time (HIP events on the compute stream) of the launches of the last
 * h9g_get_daystats; 0 before the first. */
float h9g_last_daystat_ms(h9g_ctx *ctx);
/* The same of the last h9g_get_dayquant. */
float h9g_last_dayquant_ms(h9g_ctx *ctx);
/* Digest of the sources and compile flags of this library (16 hex digits;
 * hybrid9_amd/build.py build_id).  Profiles record it, and the bench
 * attaches counters only to the build they were measured on.  No GPU. */
const char *h9g_build_id(void);

/* --- self test of the device math (h9_math.h vs glibc) ---------------- */
/* out[i] = expf(x[i]) if y == NULL, else powf(x[i], y[i]), on device. */
int h9g_math_selftest(int device, int n, const float *x, const float *y,
                      float *out);
/* The same through the year kernels' math (glibc's main path; inputs that
 * glibc sends down another path are redone in place with its full logic,
 * flag[i] = 1 there). */
int h9g_math_fast_selftest(int device, int n, const float *x, const float *y,
                           float *out, int *flag);
/* out[i] = x[i]/d[i] through the kernel's fast exact division (double
 * reciprocal); flag[i] = 1 where the quotient was redone as
 * the IEEE division (subnormal or NaN quotient). */
int h9g_div_selftest(int device, int n, const float *x, const float *d,
                     float *out, int *flag);
/* One cycle's test of h9g_spinup on hand-made states, through the same kernel
 * (h9g_spin_kernel): n cells of L layers, none masked; state_prev and state
 * are packed states (h9g_get_state's layout) one cycle apart, err (n, may be
 * NULL) the STOP code of each cell after the cycle (non-zero: it stopped in
 * it), k the cycle's number.  list (n) receives the cells still active, in
 * increasing order, cell_cycle (n) as h9g_spinup's, stats (H9G_NSPIN + 1) the
 * cycle's history row, then the list's length. */
int h9g_spin_selftest(int device, int n, int L, const float *state_prev, const float *state,
                      const int32_t *err, const h9g_spinup_opts *opts, int k,
                      int32_t *list, int32_t *cell_cycle, double *stats);
/* h9g_get_daystats on hand-made records, through the same kernel, with no
 * context and no year run: records (nt, 7, n) host, out (17, n).  nseg = 0 is
 * the product's cut of the year into slices; nseg > 0 cuts it into that many
 * (1 .. 16: the largest workgroup built) through the same code, so a test can
 * show that the cut does not matter. */
int h9g_daystat_selftest(int device, int n, int nt, int nseg, const float *records,
                         const h9g_daystat_opts *opts, double *out);
/* h9g_get_dayquant on hand-made records, through the same kernel, with no
 * context and no year run: nyears (1 .. 512) years of nt[y] (1 .. 65535) days,
 * records (nyears, ntmax, 7, n) host with ntmax = max nt, out (nres, 1 + 2 nq,
 * n).  nseg = 0 is the product's cut of a year into slices; nseg > 0 cuts
 * every year into that many (1 .. 16: the largest workgroup built) through
 * the same code, so a test can show that the cut does not matter.  Every
 * argument is checked before a device is touched. */
int h9g_dayquant_selftest(int device, int n, int nyears, const int32_t *nt, int nseg,
                          const float *records, const h9g_dayquant_opts *opts, double *out);
/* Hardware ids as the pair kernel's issue pacer decodes them: nblocks
 * workgroups of the pair kernel's shape and LDS size; per wave out[3w..3w+2]
 * = HW_REG_HW_ID, HW_REG_XCC_ID, 1 if every wave was resident at once. */
int h9g_pace_probe(int device, int nblocks, unsigned *out);

#ifdef __cplusplus
}
#endif
#endif /* H9G_H */
