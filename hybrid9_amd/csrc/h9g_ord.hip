// h9g_ord.hip -- the ordered mode: the reference's own cell order
// (h9g_run_ordered, h9g_run_decade_ordered, h9g_set_chains and their
// statistics) with its small kernels, on top of the year launch of h9g.hip
// (run_year_impl, h9g_ctx.h).  Every recording that is on (RecStream) rides
// beside the annual means: OrdDec::rec, ord_rec.  Host code and seconds to
// compile: no year kernel is instantiated here.
#include <hip/hip_runtime.h>

#include <stdio.h>

#include <algorithm>
#include <vector>

#include "h9g_ctx.h"

// Cell-order mode (h9g_run_decade_ordered).  The reference's cell loop
// (HYBRID9.f90:120-295) leaves the module array smp (SHARED.f90:198) as the
// last cell's, and the next cell's first substep reads it in beta
// (HYDROLOGY.f90:270-275).  The m land cells (context order) form chains,
// one per reference rank (h9g_set_chains); position j starts a decade from
// the smp its predecessor pred[j] holds now, or, for a chain's first cell
// (first[j]), from what the chain's last cell pred[j] held when the decade
// started.  h9g_chain_kernel compares that with the smp the cell last
// started from (guess, L rows of n), takes it over where it differs and
// flags the cell for a re-run.  st: every cell's state at the decade's end
// as known now.  dirty (may be null): cells whose decade start changed after
// the first pass ran (h9g_settle_kernel), flagged whatever their input.
__global__ void __launch_bounds__(256) h9g_chain_kernel(int m, int n, int L, const int *__restrict__ chain,
                                                        const int *__restrict__ pred, const int *__restrict__ first,
                                                        const float *__restrict__ st, const float *__restrict__ st0,
                                                        float *__restrict__ guess, const int *__restrict__ dirty,
                                                        int *__restrict__ flag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int k = chain[j];
  const float *src = first[j] ? st0 : st;
  const int p = pred[j];
  int differ = 0;
  for (int i = 0; i < L; i++) {
    // (smp_row(L, 0) + i, here and below: as smp_row(L, i), chain_start and restart take two more SGPRs)
    const float v = src[(size_t)(smp_row(L, 0) + i) * n + p];
    differ |= __float_as_uint(v) != __float_as_uint(guess[(size_t)i * n + k]);
    guess[(size_t)i * n + k] = v;
  }
  flag[j] = differ | (dirty && dirty[k] ? 2 : 0);   // 1: input changed, 2: start changed
}

// The cell order's day-1 probe (round 6).  The input smp reaches a cell only
// through beta of its decade's first substep (HYDROLOGY.f90:270-275).  A
// cell whose input changed ran the day from its old and from its new input
// (one-day list launches from the decade's start, running sums undivided,
// KArgs::raw): if the two agree bit for bit at the day's end -- every state
// row, the STOP record and every running sum of the year's means -- the
// days after it and so the whole decade are the same from either input, and
// the cell needs no re-run (its trajectory is already the one its new input
// gives).  keep[j] = 1: they differ, the cell re-runs.
__global__ void __launch_bounds__(256) h9g_probe_cmp_kernel(int m, int n, int srows, int rows,
                                                            const int *__restrict__ list,
                                                            const float *__restrict__ stA, const float *__restrict__ stB,
                                                            const int *__restrict__ errA, const int *__restrict__ errB,
                                                            const float *__restrict__ annA,
                                                            const float *__restrict__ annB, int *__restrict__ keep) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int c = list[j];
  bool same = true;
  H9K_SAME_CELL(same, stA, stB, n, c, srows);
  H9K_SAME_CELL(same, errA, errB, n, c, STOP_ROWS);
  H9K_SAME_CELL(same, annA, annB, n, c, rows);
  keep[j] = !same;
}

// Pipelined decades (h9g_run_ordered): decade D+1's first pass starts from
// every cell's state as known when decade D's first pass and year-1 re-run
// are done (st0); the cells D's later re-runs still change get their final
// D end state (fin, fin_err) here once D has settled, and are marked dirty.
// A dirty cell that has now STOPped (err0 != 0) leaves D+1: its state and
// STOP record go back into the context (st, err) and D+1's last-year
// checkpoint, and its annual means of D+1 (ny years of rows x n) are NaN.
__global__ void __launch_bounds__(256) h9g_settle_kernel(int n, int srows, int rows, int ny,
                                                         const float *__restrict__ fin, const int *__restrict__ fin_err,
                                                         float *__restrict__ st0, int *__restrict__ err0,
                                                         int *__restrict__ dirty, float *__restrict__ st,
                                                         int *__restrict__ err, float *__restrict__ ck_last,
                                                         int *__restrict__ eck_last, float *__restrict__ ann) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  bool same = true;
  H9K_SAME_CELL(same, fin, st0, n, c, srows);
  H9K_SAME_CELL(same, fin_err, err0, n, c, STOP_ROWS);
  if (same) return;
  H9K_COPY_CELL(st0, n, c, fin, n, c, srows);
  H9K_COPY_CELL(err0, n, c, fin_err, n, c, STOP_ROWS);
  dirty[c] = 1;
  if (err0[c] == 0) return;
  for (int r = 0; r < srows; r++) {
    st[(size_t)r * n + c] = st0[(size_t)r * n + c];
    ck_last[(size_t)r * n + c] = st0[(size_t)r * n + c];
  }
  for (int r = 0; r < STOP_ROWS; r++) {
    err[(size_t)r * n + c] = err0[(size_t)r * n + c];
    eck_last[(size_t)r * n + c] = err0[(size_t)r * n + c];
  }
  for (int y = 0; y < ny; y++)
    for (int r = 0; r < rows; r++) ann[((size_t)y * rows + r) * n + c] = __builtin_nanf("");
}

// Pass 0's input of every chain's first cell: the smp its chain's last cell
// holds when the decade starts (into the state and the guess).
__global__ void __launch_bounds__(256) h9g_chain_start_kernel(int m, int n, int L, const int *__restrict__ chain,
                                                              const int *__restrict__ pred, const int *__restrict__ first,
                                                              const float *__restrict__ st0, float *__restrict__ st,
                                                              float *__restrict__ guess) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m || !first[j]) return;
  const int k = chain[j], p = pred[j];
  for (int i = 0; i < L; i++) {
    const float v = st0[(size_t)(smp_row(L, 0) + i) * n + p];
    st[(size_t)(smp_row(L, 0) + i) * n + k] = v;
    guess[(size_t)i * n + k] = v;
  }
}

// The listed cells back to the decade's starting state (state rows and STOP
// record), starting from the smp in guess.
__global__ void __launch_bounds__(256) h9g_restart_kernel(int m, int n, int L, const int *__restrict__ list,
                                                          const float *__restrict__ st0, const int *__restrict__ err0,
                                                          const float *__restrict__ guess, float *__restrict__ st,
                                                          int *__restrict__ err) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int k = list[j];
  const int rows = state_rows(L);
  H9K_COPY_CELL(st, n, k, st0, n, k, rows);
  for (int i = 0; i < L; i++) st[(size_t)(smp_row(L, 0) + i) * n + k] = guess[(size_t)i * n + k];
  H9K_COPY_CELL(err, n, k, err0, n, k, STOP_ROWS);
}

// A re-run cell's trajectory against the one its last run took (ckpt: the
// state and STOP record at the end of the same year).  The state and the
// STOP record are everything a year carries into the next (the c4_spinup
// decade carry), so a cell whose end-of-year state equals the old one's bit
// for bit runs the rest of the decade exactly as it did: it leaves the
// re-run with the old run's end-of-decade state (ckpt_last), its later
// annual means stand, and keep[j] = 0.  Otherwise its new state becomes the
// checkpoint and it runs on (keep[j] = 1).
__global__ void __launch_bounds__(256) h9g_merge_kernel(int m, int n, int rows, const int *__restrict__ list,
                                                        float *__restrict__ st, int *__restrict__ err,
                                                        float *__restrict__ ckpt, int *__restrict__ eckpt,
                                                        const float *__restrict__ ckpt_last,
                                                        const int *__restrict__ eckpt_last, int *__restrict__ keep) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int k = list[j];
  bool same = true;
  H9K_SAME_CELL(same, st, ckpt, n, k, rows);
  H9K_SAME_CELL(same, err, eckpt, n, k, STOP_ROWS);
  if (same) {
    H9K_COPY_CELL(st, n, k, ckpt_last, n, k, rows);
    H9K_COPY_CELL(err, n, k, eckpt_last, n, k, STOP_ROWS);
  } else {
    H9K_COPY_CELL(ckpt, n, k, st, n, k, rows);
    H9K_COPY_CELL(eckpt, n, k, err, n, k, STOP_ROWS);
  }
  keep[j] = !same;
}

extern "C" {

// ---------------------------------------------------------------------------
// The reference's own cell order (h9g_run_ordered, h9g_run_decade_ordered)
// ---------------------------------------------------------------------------
// One decade of the reference's loop (HYBRID9.f90:93-130) is a fixed point
// on the device.  Pass 0 runs every cell's years from its own smp.
// h9g_chain_kernel then gives every land cell the smp its predecessor now
// ends the decade with and flags the cells whose input changed; those
// re-run from the decade's starting state (h9g_restart_kernel), and the pass
// repeats until no input changes.  A cell's result depends on its
// predecessor's only through that smp, so when no input changes every cell
// has run from the input the reference gives it.  Position p of a chain is
// exact after pass p + 1 at the latest: at most m + 1 passes.
//
// A re-run stops early.  The input smp reaches a cell's decade only through
// beta of its first substep (HYDROLOGY.f90:270-275), and the perturbation
// it starts is rounded away within months in most cells: from then on the
// cell runs bit for bit as before.  Every run therefore checkpoints each
// cell's state and STOP record at every year end (ck), and after each
// re-run year h9g_merge_kernel drops the cells whose state is the
// checkpoint's again: they keep the old trajectory's later years and end
// state (and so the input their successor already has).  Pass 1 then costs
// about one year for most cells instead of ten.
//
// Decades overlap (round 6).  Decade D+1's first pass needs only every
// cell's own end state of D, which the first pass of D gives for every cell
// the re-runs leave alone; so it starts as soon as D's first pass and the
// re-run of year 1 (every cell whose input changed) are done.  D's
// remaining re-runs -- a tail of a few dozen cells whose perturbation
// lasts, run year by year -- ride as a second group of waves in D+1's year
// launches (KArgs::split, on their own state rows st2), in the slots the
// grid leaves free in the launch's last round of resident workgroups.  Once
// D has settled, the cells whose end of D differs from where D+1's first
// pass started them get their final state (h9g_settle_kernel) and are
// re-run in D+1's first check whatever their input.  Each decade's first
// pass, checkpoints and re-runs read only its own buffers (OrdDec), so D's
// tail and D+1's first pass are independent.
struct OrdDec {
  int y0 = 0, ny = 0, k0 = 0;            // first year, years, index of its first year in the call
  float *st0 = nullptr, *guess = nullptr, *ann = nullptr, *ck = nullptr;
  float *rec[REC_N] = {};                // the recordings beside ann, each (years, its rows of a year, n); null
  int rec_cap = 0;                       // until its stream is on in a call (ord_rec_alloc); years of each
  int *err0 = nullptr, *eck = nullptr, *dirty = nullptr;
  int *d_chain = nullptr, *d_pred = nullptr, *d_first = nullptr, *d_list = nullptr, *d_flag = nullptr;
  std::vector<int> chain, list, flag;
  int m = 0;
  enum { PASS0, CHECK, RERUN, SETTLED } phase = PASS0;
  int next_y = 0, np = 0;
};

struct OrdBufs {
  OrdDec d[2];
  float *st2 = nullptr;                  // the re-running cells' state and STOP rows
  int *err2 = nullptr;
  int *d_bulk = nullptr;                 // a first pass's cells when some are left out of it
  // the day-1 probe (h9g_probe_cmp_kernel): the inputs the checked cells'
  // trajectories started from, the probe list and its two runs
  float *gold = nullptr, *pst = nullptr, *pann = nullptr;
  int *perr = nullptr, *d_plist = nullptr, *d_pkeep = nullptr;
  int ny_cap = 0;
};

void ord_free(h9g_ctx *ctx) {
  OrdBufs *o = ctx->ord;
  if (!o) return;
  for (OrdDec &D : o->d) {
    for (float *p : {D.st0, D.guess, D.ann, D.ck}) (void)hipFree(p);
    for (float *p : D.rec) (void)hipFree(p);
    for (int *p : {D.err0, D.eck, D.dirty, D.d_chain, D.d_pred, D.d_first, D.d_list, D.d_flag}) (void)hipFree(p);
  }
  (void)hipFree(o->st2);
  (void)hipFree(o->err2);
  (void)hipFree(o->d_bulk);
  for (float *p : {o->gold, o->pst, o->pann}) (void)hipFree(p);
  for (int *p : {o->perr, o->d_plist, o->d_pkeep}) (void)hipFree(p);
  delete o;
  ctx->ord = nullptr;
}

static int ord_alloc(h9g_ctx *ctx, int ny) {
  if (ctx->ord && ctx->ord->ny_cap >= ny) return 0;
  ord_free(ctx);
  ctx->ord = new OrdBufs();
  OrdBufs *o = ctx->ord;
  const size_t n = ctx->n, L = (size_t)ctx->L, srows = (size_t)h9g_state_size(ctx->L), rows = annual_rows(ctx->L);
  bool ok = hipMalloc(&o->st2, sizeof(float) * srows * n) == hipSuccess &&
            hipMalloc(&o->err2, sizeof(int) * STOP_ROWS * n) == hipSuccess &&
            hipMalloc(&o->d_bulk, sizeof(int) * (n + 1)) == hipSuccess &&
            hipMalloc(&o->gold, sizeof(float) * L * n) == hipSuccess &&
            hipMalloc(&o->pst, sizeof(float) * 2 * srows * n) == hipSuccess &&
            hipMalloc(&o->pann, sizeof(float) * 2 * rows * n) == hipSuccess &&
            hipMalloc(&o->perr, sizeof(int) * 2 * STOP_ROWS * n) == hipSuccess &&
            hipMalloc(&o->d_plist, sizeof(int) * (n + 1)) == hipSuccess &&
            hipMalloc(&o->d_pkeep, sizeof(int) * (n + 1)) == hipSuccess;
  for (OrdDec &D : o->d) {
    ok = ok && hipMalloc(&D.st0, sizeof(float) * srows * n) == hipSuccess &&
         hipMalloc(&D.guess, sizeof(float) * L * n) == hipSuccess &&
         hipMalloc(&D.ann, sizeof(float) * (size_t)ny * rows * n) == hipSuccess &&
         hipMalloc(&D.ck, sizeof(float) * (size_t)ny * srows * n) == hipSuccess &&
         hipMalloc(&D.err0, sizeof(int) * STOP_ROWS * n) == hipSuccess &&
         hipMalloc(&D.eck, sizeof(int) * (size_t)ny * STOP_ROWS * n) == hipSuccess &&
         hipMalloc(&D.dirty, sizeof(int) * n) == hipSuccess;
    for (int **p : {&D.d_chain, &D.d_pred, &D.d_first, &D.d_list, &D.d_flag})
      ok = ok && hipMalloc(p, sizeof(int) * (n + 1)) == hipSuccess;
  }
  if (!ok) {
    ord_free(ctx);
    return H9G_ENOMEM;
  }
  o->ny_cap = ny;
  return 0;
}

// Work counters of the last ordered call (h9g_decade_stats, h9g_ordered_stats).
struct OrdStats {
  int64_t passes = 0, rerun_cells = 0, rerun_cell_years = 0, rerun_launches = 0;
  int64_t ticks = 0, ride_steps = 0, ride_cell_years = 0, alone_steps = 0, alone_cell_years = 0, excluded = 0;
  int64_t probed = 0, probe_kept = 0;
  std::vector<int64_t> launch_cells, dec_passes;
};

static float *ord_ck(const h9g_ctx *ctx, const OrdDec &D, int y) {
  return D.ck + (size_t)y * h9g_state_size(ctx->L) * ctx->n;
}
static int *ord_eck(const h9g_ctx *ctx, const OrdDec &D, int y) { return D.eck + (size_t)y * STOP_ROWS * ctx->n; }
static float *ord_ann(const h9g_ctx *ctx, const OrdDec &D, int y) { return D.ann + (size_t)y * annual_rows(ctx->L) * ctx->n; }
// The rows of recording `which` (RecStream) of a decade's year: they live
// beside its annual rows, and every launch that writes the one writes the
// other (null with that recording off).
static float *ord_rec(const h9g_ctx *ctx, const OrdDec &D, int which, int y) {
  const RecStream &s = ctx->rec[which];
  return s.on ? D.rec[which] + (size_t)y * s.year_floats(ctx->n) : nullptr;
}
// Room for ny years of every recording that is on, in both decades' buffers.
// A decade's buffers all hold rec_cap years: to grow, all of them go.
static int ord_rec_alloc(h9g_ctx *ctx, int ny) {
  for (OrdDec &D : ctx->ord->d) {
    if (D.rec_cap < ny) {
      for (float *&p : D.rec) {
        (void)hipFree(p);
        p = nullptr;
      }
      D.rec_cap = ny;
    }
    for (int w = 0; w < REC_N; w++)
      if (ctx->rec[w].on && !D.rec[w])
        if (int r = rec_malloc(&D.rec[w], (size_t)D.rec_cap * ctx->rec[w].year_floats(ctx->n))) return r;
  }
  return 0;
}

// The decade's chains (h9g_set_chains) over its land cells that have not
// stopped when it starts (its final err0), in context order: predecessors
// are the previous land cell of the same chain, for a chain's first cell its
// last one.
static int ord_chain(h9g_ctx *ctx, OrdDec &D, const std::vector<char> &land) {
  const size_t n = ctx->n;
  std::vector<int> e0(n);
  HIPCHK(hipStreamSynchronize(ctx->sc));   // (the compute stream is non-blocking: hipMemcpy does not wait for it)
  HIPCHK(hipMemcpy(e0.data(), D.err0, sizeof(int) * n, hipMemcpyDeviceToHost));
  D.chain.clear();
  for (size_t c = 0; c < n; c++)
    if (land[c] && e0[c] == 0) D.chain.push_back((int)c);
  const int m = D.m = (int)D.chain.size();
  std::vector<int> pred(m), first(m), last_of, first_of;
  auto cid = [&](int j) { return ctx->chain_id.empty() ? 0 : ctx->chain_id[(size_t)D.chain[j]]; };
  for (int j = 0; j < m; j++) {
    const int c = cid(j);
    if ((int)last_of.size() <= c) {
      last_of.resize((size_t)c + 1, -1);
      first_of.resize((size_t)c + 1, -1);
    }
    if (last_of[(size_t)c] < 0) {
      first_of[(size_t)c] = j;
      first[j] = 1;
    } else {
      pred[j] = D.chain[last_of[(size_t)c]];
      first[j] = 0;
    }
    last_of[(size_t)c] = j;
  }
  for (int j = 0; j < m; j++)
    if (first[j]) pred[j] = D.chain[last_of[(size_t)cid(j)]];
  if (m > 0) {
    HIPCHK(hipMemcpy(D.d_chain, D.chain.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.d_pred, pred.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.d_first, first.data(), sizeof(int) * m, hipMemcpyHostToDevice));
  }
  D.flag.assign((size_t)m + 1, 0);
  return 0;
}

// A check of decade D: every chain cell's input from its predecessor's end
// of the decade as known now (the last year's checkpoint); the flagged cells
// back to the decade's start on the re-run rows st2 (phase RERUN), or, with
// none flagged, D has settled.
// The day-1 probe of the cells in `cand` (their input changed, their start
// did not): each runs its decade's first day from the smp its trajectory
// started from (o->gold) and from its new one (D.guess); the cells whose two
// days differ are appended to D.list (h9g_probe_cmp_kernel).
static int ord_probe(h9g_ctx *ctx, OrdDec &D, const int32_t *slots, const std::vector<int> &cand, OrdStats &S) {
  OrdBufs *o = ctx->ord;
  const int n = (int)ctx->n, L = ctx->L, k = (int)cand.size();
  const int rows = annual_rows(L), srows = h9g_state_size(L);
  HIPCHK(hipMemcpyAsync(o->d_plist, cand.data(), sizeof(int) * k, hipMemcpyHostToDevice, ctx->sc));
  for (int v = 0; v < 2; v++) {
    float *st = o->pst + (size_t)v * srows * n;
    int *err = o->perr + (size_t)v * STOP_ROWS * n;
    h9g_restart_kernel<<<(unsigned)((k + 255) / 256), 256, 0, ctx->sc>>>(k, n, L, o->d_plist, D.st0, D.err0,
                                                                        v ? D.guess : o->gold, st, err);
    HIPCHK(hipGetLastError());
    YearSpec ys;
    ys.slot = slots[D.k0];
    ys.jyear = D.y0;
    ys.d_list = o->d_plist;
    ys.m = k;
    ys.ann_dst = o->pann + (size_t)v * rows * n;
    ys.st = st;
    ys.err = err;
    ys.ndays = 1;
    ys.probe = true;
    if (int r = run_year_impl(ctx, ys)) return r;
  }
  h9g_probe_cmp_kernel<<<(unsigned)((k + 255) / 256), 256, 0, ctx->sc>>>(
      k, n, srows, rows, o->d_plist, o->pst, o->pst + (size_t)srows * n, o->perr, o->perr + (size_t)STOP_ROWS * n, o->pann,
      o->pann + (size_t)rows * n, o->d_pkeep);
  HIPCHK(hipGetLastError());
  std::vector<int> keep(k);
  HIPCHK(hipMemcpyAsync(keep.data(), o->d_pkeep, sizeof(int) * k, hipMemcpyDeviceToHost, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  int kept = 0;
  for (int j = 0; j < k; j++)
    if (keep[j]) {
      D.list.push_back(cand[j]);
      kept++;
    }
  S.probed += k;
  S.probe_kept += kept;
  return 0;
}

static int ord_check(h9g_ctx *ctx, OrdDec &D, const int32_t *slots, bool use_dirty, OrdStats &S) {
  OrdBufs *o = ctx->ord;
  const int n = (int)ctx->n, L = ctx->L, m = D.m;
  D.list.clear();
  if (m > 0) {
    // the inputs the trajectories started from, for the probe
    HIPCHK(hipMemcpyAsync(o->gold, D.guess, sizeof(float) * L * n, hipMemcpyDeviceToDevice, ctx->sc));
    h9g_chain_kernel<<<(unsigned)((m + 255) / 256), 256, 0, ctx->sc>>>(m, n, L, D.d_chain, D.d_pred, D.d_first,
                                                                      ord_ck(ctx, D, D.ny - 1), D.st0, D.guess,
                                                                      use_dirty ? D.dirty : nullptr, D.d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.flag.data(), D.d_flag, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->sc));
    HIPCHK(hipStreamSynchronize(ctx->sc));
    std::vector<int> cand;
    const bool probe = ctx->ord_probe;
    for (int j = 0; j < m; j++) {
      if (probe && D.flag[j] == 1)
        cand.push_back(D.chain[j]);
      else if (D.flag[j])
        D.list.push_back(D.chain[j]);
    }
    if (!cand.empty()) {
      if (int r = ord_probe(ctx, D, slots, cand, S)) return r;
      std::sort(D.list.begin(), D.list.end());
    }
  }
  if (D.list.empty()) {
    D.phase = OrdDec::SETTLED;
    return 0;
  }
  if (D.np > m + 1) return H9G_ESTATE;   // cannot happen (see above): a broken invariant, not a result
  const int k = (int)D.list.size();
  HIPCHK(hipMemcpy(D.d_list, D.list.data(), sizeof(int) * k, hipMemcpyHostToDevice));
  h9g_restart_kernel<<<(unsigned)((k + 255) / 256), 256, 0, ctx->sc>>>(k, n, L, D.d_list, D.st0, D.err0, D.guess,
                                                                      o->st2, o->err2);
  HIPCHK(hipGetLastError());
  S.rerun_cells += k;
  D.next_y = 0;
  D.phase = OrdDec::RERUN;
  return 0;
}

// After a re-run year of decade D's list: the cells back on their old
// trajectory leave the re-run (h9g_merge_kernel); at the decade's end, or
// with none left, the pass ends and a check follows.
static int ord_after_run(h9g_ctx *ctx, OrdDec &D, OrdStats &S) {
  OrdBufs *o = ctx->ord;
  const int n = (int)ctx->n, srows = h9g_state_size(ctx->L);
  const int k = (int)D.list.size(), y = D.next_y;
  h9g_merge_kernel<<<(unsigned)((k + 255) / 256), 256, 0, ctx->sc>>>(k, n, srows, D.d_list, o->st2, o->err2,
                                                                    ord_ck(ctx, D, y), ord_eck(ctx, D, y),
                                                                    ord_ck(ctx, D, D.ny - 1), ord_eck(ctx, D, D.ny - 1),
                                                                    D.d_flag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(D.flag.data(), D.d_flag, sizeof(int) * k, hipMemcpyDeviceToHost, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  S.rerun_cell_years += k;
  S.rerun_launches++;
  S.launch_cells.push_back(k);
  int kk = 0;
  for (int j = 0; j < k; j++)
    if (D.flag[j]) D.list[kk++] = D.list[j];
  D.list.resize(kk);
  if (kk > 0 && kk < k) HIPCHK(hipMemcpy(D.d_list, D.list.data(), sizeof(int) * kk, hipMemcpyHostToDevice));
  D.next_y = y + 1;
  if (kk == 0 || D.next_y == D.ny) {
    D.np++;
    D.phase = OrdDec::CHECK;
  }
  return 0;
}

// One re-run year of decade D's list as a launch of its own.
static int ord_run_alone(h9g_ctx *ctx, OrdDec &D, const int32_t *slots, OrdStats &S) {
  YearSpec ys;
  ys.slot = slots[D.k0 + D.next_y];
  ys.jyear = D.y0 + D.next_y;
  ys.d_list = D.d_list;
  ys.m = (int)D.list.size();
  ys.ann_dst = ord_ann(ctx, D, D.next_y);
  for (int w = 0; w < REC_N; w++) ys.rec_dst[w] = ord_rec(ctx, D, w, D.next_y);
  ys.st = ctx->ord->st2;
  ys.err = ctx->ord->err2;
  if (int r = run_year_impl(ctx, ys)) return r;
  S.alone_steps++;
  S.alone_cell_years += ys.m;
  return ord_after_run(ctx, D, S);
}

// Runs D's checks and re-runs until it has settled.
static int ord_settle(h9g_ctx *ctx, OrdDec &D, const int32_t *slots, OrdStats &S) {
  while (D.phase != OrdDec::SETTLED) {
    const int r = D.phase == OrdDec::CHECK ? ord_check(ctx, D, slots, false, S) : ord_run_alone(ctx, D, slots, S);
    if (r) return r;
  }
  return 0;
}

// D has settled: its annual means to the host, its first new STOP into the
// context's error record, and -- with a next decade N under way -- its end
// states into N's start (h9g_settle_kernel).
static int ord_finish(h9g_ctx *ctx, OrdDec &D, OrdDec *N, float *annual, int &stop_seen) {
  const size_t n = ctx->n;
  const int rows = annual_rows(ctx->L), srows = h9g_state_size(ctx->L);
  if (annual)
    HIPCHK(hipMemcpyAsync(annual + (size_t)D.k0 * rows * n, D.ann, sizeof(float) * (size_t)D.ny * rows * n,
                          hipMemcpyDeviceToHost, ctx->sc));
  if (!stop_seen && ctx->last_err.code == 0) {
    std::vector<int> e0(n), e1(STOP_ROWS * n);
    HIPCHK(hipMemcpyAsync(e0.data(), D.err0, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->sc));
    HIPCHK(hipMemcpyAsync(e1.data(), ord_eck(ctx, D, D.ny - 1), sizeof(int) * STOP_ROWS * n, hipMemcpyDeviceToHost, ctx->sc));
    HIPCHK(hipStreamSynchronize(ctx->sc));
    for (size_t c = 0; c < n; c++) {
      if (e1[c] == 0 || e0[c] != 0) continue;
      // the first cell in context order to STOP in this decade, in the first
      // year of the decade whose means it has not completed
      std::vector<float> npp(D.ny);
      for (int y = 0; y < D.ny; y++)
        HIPCHK(hipMemcpy(&npp[y], ord_ann(ctx, D, y) + c, sizeof(float), hipMemcpyDeviceToHost));
      int y = 0;
      while (y < D.ny - 1 && npp[y] == npp[y]) y++;
      ctx->last_err.code = e1[c];
      ctx->last_err.cell = (int)c;
      ctx->last_err.year = D.y0 + y;
      ctx->last_err.day = e1[n + c];
      ctx->last_err.substep = e1[2 * n + c];
      ctx->last_err.value = __builtin_bit_cast(float, e1[3 * n + c]);
      stop_seen = 1;
      break;
    }
  }
  for (int w = 0; w < REC_N; w++)   // the settled decade's recordings into the call's retained buffers
    if (const RecStream &s = ctx->rec[w]; s.on)
      HIPCHK(hipMemcpyAsync(s.ret_year(n, s.base + D.k0), D.rec[w], sizeof(float) * (size_t)D.ny * s.year_floats(n),
                            hipMemcpyDeviceToDevice, ctx->sc));
  if (N) {
    h9g_settle_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->sc>>>(
        (int)n, srows, rows, N->ny, ord_ck(ctx, D, D.ny - 1), ord_eck(ctx, D, D.ny - 1), N->st0, N->err0, N->dirty,
        ctx->d_st, ctx->d_err, ord_ck(ctx, *N, N->ny - 1), ord_eck(ctx, *N, N->ny - 1), N->ann);
    // NaN recorded rows where it wrote NaN means: a cell that starts N stopped runs
    // none of N's years (N's first pass is done, and its chains leave it out)
    for (int w = 0; w < REC_N; w++)
      if (ctx->rec[w].on)
        h9g_nan_stopped_rows((int)n, N->ny * (int)ctx->rec[w].year_rows, N->err0, N->rec[w], ctx->sc);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->sc));
  return 0;
}

// Cells left out of a decade's first pass (still re-running the decade
// before): re-run in its first check whatever their input (dirty), and never
// merged back onto a first-pass trajectory they did not run (their
// checkpoints' STOP code -1, which no run produces).
__global__ void __launch_bounds__(256) h9g_exclude_kernel(int k, int n, int ny, const int *__restrict__ list,
                                                          int *__restrict__ dirty, int *__restrict__ eck) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int c = list[j];
  dirty[c] = 1;
  for (int y = 0; y < ny; y++) eck[(size_t)y * STOP_ROWS * n + c] = -1;
}

// decades: (first year, years) of each decade the call runs, in order;
// their years' forcing in slots[0 .. sum of years).
static int run_ordered_impl(h9g_ctx *ctx, const int32_t *slots, int jyear0,
                            const std::vector<std::pair<int, int>> &decs, float *annual, int32_t *passes) {
  if (!ctx || !slots || decs.empty()) return H9G_EINVAL;
  int nyears = 0, nymax = 0;
  for (auto &d : decs) {
    nyears += d.second;
    nymax = std::max(nymax, d.second);
  }
  if (nyears < 1 || nymax > ctx->cfg.nslots) return H9G_EINVAL;
  for (int y = 0; y < nyears; y++)
    if (slots[y] < 0 || slots[y] >= ctx->cfg.nslots || jyear0 + y < 1861 || jyear0 + y > 2299) return H9G_EINVAL;
  {
    // every year its own slot: a decade's re-runs read their years' forcing
    // while the next decade's first pass reads its own
    std::vector<char> used((size_t)ctx->cfg.nslots, 0);
    for (int y = 0; y < nyears; y++)
      if (used[(size_t)slots[y]]++) return H9G_EINVAL;
  }
  if (!ctx->params_set || !ctx->state_set) return H9G_ESTATE;
  const size_t n = ctx->n;
  const int L = ctx->L, rows = annual_rows(L), srows = h9g_state_size(L);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  if (int r = ord_alloc(ctx, nymax)) return r;
  if (int r = ord_rec_alloc(ctx, nymax)) return r;
  OrdBufs *o = ctx->ord;
  // land cells (HYBRID9.f90:122-123, summed in layer order as the year
  // kernels do)
  std::vector<char> land(n);
  {
    std::vector<float> ts((size_t)L * n);
    HIPCHK(hipMemcpy(ts.data(), ctx->d_par, sizeof(float) * ts.size(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < n; c++) {
      float sum = 0.0f;
      for (int i = 0; i < L; i++) sum = sum + ts[(size_t)i * n + c];
      land[c] = sum > 1.0E-8f;
    }
  }
  OrdStats S;
  int stop_seen = 0;
  OrdDec *P = nullptr;                     // the decade whose re-runs are still going
  int k0 = 0;
  for (size_t i = 0; i < decs.size(); i++) {
    OrdDec &D = o->d[i & 1];
    D.y0 = decs[i].first;
    D.ny = decs[i].second;
    D.k0 = k0;
    k0 += D.ny;
    D.phase = OrdDec::PASS0;
    D.np = 0;
    D.next_y = 0;
    D.list.clear();
    // the decade starts from the context's state as known now
    HIPCHK(hipMemcpyAsync(D.st0, ctx->d_st, sizeof(float) * srows * n, hipMemcpyDeviceToDevice, ctx->sc));
    HIPCHK(hipMemcpyAsync(D.err0, ctx->d_err, sizeof(int) * STOP_ROWS * n, hipMemcpyDeviceToDevice, ctx->sc));
    HIPCHK(hipMemcpyAsync(D.guess, ctx->d_st + (size_t)smp_row(L, 0) * n, sizeof(float) * (size_t)L * n,
                          hipMemcpyDeviceToDevice, ctx->sc));
    HIPCHK(hipMemsetAsync(D.dirty, 0, sizeof(int) * n, ctx->sc));
    // the cells P is still re-running stay out of D's first pass: their end
    // of P, D's start, is not known yet (they re-run D in its first check);
    // the others form the first pass's list, and P's re-runs ride in its
    // launches in the slots this leaves
    std::vector<int> excl;
    if (P && P->phase == OrdDec::RERUN && !ctx->no_exclude) {
      excl = P->list;
      std::sort(excl.begin(), excl.end());
    }
    int nb = (int)n;
    if (!excl.empty()) {
      std::vector<int> bulk;
      bulk.reserve(n - excl.size());
      size_t e = 0;
      for (int c = 0; c < (int)n; c++) {
        if (e < excl.size() && excl[e] == c) {
          e++;
          continue;
        }
        bulk.push_back(c);
      }
      nb = (int)bulk.size();
      HIPCHK(hipMemcpy(o->d_bulk, bulk.data(), sizeof(int) * nb, hipMemcpyHostToDevice));
    }
    S.excluded += (int64_t)excl.size();
    // pass 0: each year one launch, P's re-runs riding along
    for (int y = 0; y < D.ny; y++) {
      YearSpec ys;
      ys.slot = slots[D.k0 + y];
      ys.jyear = D.y0 + y;
      if (!excl.empty()) {
        ys.d_list = o->d_bulk;
        ys.m = nb;
        ys.bulk = true;
        ys.ann_dst = ctx->d_ann;
        for (int w = 0; w < REC_N; w++) ys.rec_dst[w] = ctx->rec[w].d_year;
      }
      const bool ride = P && P->phase == OrdDec::RERUN && g2_fits(ctx, (size_t)nb, P->list.size()) &&
                        !ctx->no_ride;
      if (ride) {
        ys.h2 = P->list.data();
        ys.k2 = (int)P->list.size();
        ys.slot2 = slots[P->k0 + P->next_y];
        ys.jyear2 = P->y0 + P->next_y;
        ys.st2 = o->st2;
        ys.err2 = o->err2;
        ys.ann2 = ord_ann(ctx, *P, P->next_y);
        for (int w = 0; w < REC_N; w++) ys.rec2[w] = ord_rec(ctx, *P, w, P->next_y);
      }
      if (int r = run_year_impl(ctx, ys)) return r;
      S.ticks++;
      HIPCHK(hipMemcpyAsync(ord_ann(ctx, D, y), ctx->d_ann, sizeof(float) * rows * n, hipMemcpyDeviceToDevice, ctx->sc));
      for (int w = 0; w < REC_N; w++)
        if (const RecStream &s = ctx->rec[w]; s.on)
          HIPCHK(hipMemcpyAsync(ord_rec(ctx, D, w, y), s.d_year, sizeof(float) * s.year_floats(n), hipMemcpyDeviceToDevice,
                                ctx->sc));
      HIPCHK(hipMemcpyAsync(ord_ck(ctx, D, y), ctx->d_st, sizeof(float) * srows * n, hipMemcpyDeviceToDevice, ctx->sc));
      HIPCHK(hipMemcpyAsync(ord_eck(ctx, D, y), ctx->d_err, sizeof(int) * STOP_ROWS * n, hipMemcpyDeviceToDevice, ctx->sc));
      if (ride) {
        S.ride_steps++;
        S.ride_cell_years += ys.k2;
        if (int r = ord_after_run(ctx, *P, S)) return r;
      }
      if (P && P->phase == OrdDec::CHECK)    // P's next pass starts in time for the next launch
        if (int r = ord_check(ctx, *P, slots, false, S)) return r;
    }
    D.np = 1;
    if (!excl.empty()) {
      HIPCHK(hipMemcpy(D.d_list, excl.data(), sizeof(int) * excl.size(), hipMemcpyHostToDevice));
      h9g_exclude_kernel<<<(unsigned)((excl.size() + 255) / 256), 256, 0, ctx->sc>>>((int)excl.size(), (int)n, D.ny,
                                                                                    D.d_list, D.dirty, D.eck);
      HIPCHK(hipGetLastError());
    }
    if (P) {                                 // P's remaining re-runs, then its end into D's start
      if (int r = ord_settle(ctx, *P, slots, S)) return r;
      if (int r = ord_finish(ctx, *P, &D, annual, stop_seen)) return r;
      S.dec_passes.push_back(P->np);
      S.passes += P->np;
    }
    // D's first check (its cells whose start changed flagged too) and the
    // year-1 re-run of every cell whose input changed
    if (int r = ord_chain(ctx, D, land)) return r;
    if (int r = ord_check(ctx, D, slots, true, S)) return r;
    if (D.phase == OrdDec::RERUN)
      if (int r = ord_run_alone(ctx, D, slots, S)) return r;
    if (D.phase == OrdDec::CHECK)
      if (int r = ord_check(ctx, D, slots, false, S)) return r;
    P = &D;
  }
  if (int r = ord_settle(ctx, *P, slots, S)) return r;
  if (int r = ord_finish(ctx, *P, nullptr, annual, stop_seen)) return r;
  S.dec_passes.push_back(P->np);
  S.passes += P->np;
  // daily diagnostics (h9g_set_daily): the decade has settled, so guess holds
  // the smp every chain cell's first substep reads; the selected cells run the
  // decade once more from its start (st0, err0) with that input
  if (!ctx->daily_sel.empty()) {
    if (decs.size() != 1) return H9G_EINVAL;   // (h9g_run_ordered runs its decades one by one then)
    if (int r = daily_launch(ctx, P->st0, P->guess, P->err0, slots + P->k0, P->y0, P->ny)) return r;
  }
  // the last decade's end: the context's state, STOP records and last-year means
  HIPCHK(hipMemcpyAsync(ctx->d_st, ord_ck(ctx, *P, P->ny - 1), sizeof(float) * srows * n, hipMemcpyDeviceToDevice,
                        ctx->sc));
  HIPCHK(hipMemcpyAsync(ctx->d_err, ord_eck(ctx, *P, P->ny - 1), sizeof(int) * STOP_ROWS * n, hipMemcpyDeviceToDevice, ctx->sc));
  HIPCHK(hipMemcpyAsync(ctx->d_ann, ord_ann(ctx, *P, P->ny - 1), sizeof(float) * rows * n, hipMemcpyDeviceToDevice,
                        ctx->sc));
  if (int r = diag_launch(ctx)) return r;
  ctx->last_year = P->y0 + P->ny - 1;
  if (passes)
    for (size_t i = 0; i < S.dec_passes.size(); i++) passes[i] = (int32_t)S.dec_passes[i];
  ctx->dec_stats[0] = S.passes;
  ctx->dec_stats[1] = S.rerun_cells;
  ctx->dec_stats[2] = S.rerun_cell_years;
  ctx->dec_stats[3] = S.rerun_launches;
  ctx->dec_launches = S.launch_cells;
  const int64_t os[9] = {(int64_t)decs.size(), S.ticks, S.ride_steps, S.ride_cell_years, S.alone_steps,
                         S.alone_cell_years, S.excluded, S.probed, S.probe_kept};
  std::copy(os, os + 9, ctx->ord_stats);
  ctx->ord_passes = S.dec_passes;
  for (RecStream &s : ctx->rec) {
    if (!s.on) continue;
    s.nt.resize((size_t)s.base);
    for (int y = 0; y < nyears; y++) s.nt.push_back(days_in_year(jyear0 + y));
    s.in_ret = true;
  }
  // the first STOP of the call (h9g_last_error) or one from before it
  return h9g_sync(ctx);
}

// The reference's decades (HYBRID9.f90:93-113: 1901-1910, 1911-1920, ...)
// cut to [jyear0, jyear0 + nyears).
static std::vector<std::pair<int, int>> ref_decades(int jyear0, int nyears) {
  std::vector<std::pair<int, int>> out;
  for (int y = jyear0, end = jyear0 + nyears; y < end;) {
    const int d = y - 1901, start = 1901 + 10 * (d >= 0 ? d / 10 : -((9 - d) / 10));
    const int e = std::min(start + 10, end);
    out.push_back({y, e - y});
    y = e;
  }
  return out;
}

int h9g_run_decade_ordered(h9g_ctx *ctx, const int32_t *slots, int jyear0, int nyears, float *annual, int32_t *passes) {
  if (nyears < 1) return H9G_EINVAL;
  if (ctx && !ctx->daily_sel.empty()) {
    if (jyear0 < 1861 || jyear0 + nyears - 1 > 2299) return H9G_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (int r = daily_begin(ctx, jyear0, nyears)) return r;
  }
  if (ctx)
    if (int r = rec_begin(ctx, nyears)) return r;
  return run_ordered_impl(ctx, slots, jyear0, {{jyear0, nyears}}, annual, passes);
}

int h9g_run_ordered(h9g_ctx *ctx, const int32_t *slots, int jyear0, int nyears, float *annual, int32_t *passes) {
  if (nyears < 1 || jyear0 < 1861) return H9G_EINVAL;
  if (ctx)
    if (int r = rec_begin(ctx, nyears)) return r;
  if (ctx && !ctx->daily_sel.empty()) {
    // with a selection the decades run one after another, each as
    // h9g_run_decade_ordered runs it (the same results bit for bit), and each
    // replays the selected cells once it has settled
    if (!slots || jyear0 + nyears - 1 > 2299) return H9G_EINVAL;
    std::vector<char> used((size_t)ctx->cfg.nslots, 0);
    for (int y = 0; y < nyears; y++)
      if (slots[y] < 0 || slots[y] >= ctx->cfg.nslots || used[(size_t)slots[y]]++) return H9G_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (int r = daily_begin(ctx, jyear0, nyears)) return r;
    const size_t rows = annual_rows(ctx->L);
    int first = 0, k0 = 0, i = 0;
    for (const auto &d : ref_decades(jyear0, nyears)) {
      for (RecStream &s : ctx->rec) s.base = k0;
      const int r = run_ordered_impl(ctx, slots + k0, d.first, {d}, annual ? annual + (size_t)k0 * rows * ctx->n : nullptr,
                                     passes ? passes + i : nullptr);
      if (r < 0) return r;
      if (r > 0 && !first) first = r;
      k0 += d.second;
      i++;
    }
    return first;
  }
  return run_ordered_impl(ctx, slots, jyear0, ref_decades(jyear0, nyears), annual, passes);
}

int h9g_set_chains(h9g_ctx *ctx, const int32_t *chain) {
  if (!ctx) return H9G_EINVAL;
  if (!chain) {
    ctx->chain_id.clear();
    return 0;
  }
  for (size_t c = 0; c < ctx->n; c++)
    if (chain[c] < 0 || chain[c] >= (int32_t)ctx->n) {
      fprintf(stderr, "h9g_set_chains: cell %zu has chain id %d, not in [0, ncell): cells outside every reference "
                      "block (shard.reference_blocks gives -1) belong to no rank's run and must be left out of the "
                      "context\n", c, (int)chain[c]);
      return H9G_EINVAL;
    }
  ctx->chain_id.assign(chain, chain + ctx->n);
  return 0;
}

int h9g_decade_stats(h9g_ctx *ctx, int64_t *out, int n) {
  if (!ctx || !out || n < 1) return H9G_EINVAL;
  int m = 0;
  for (; m < n && m < 4; m++) out[m] = ctx->dec_stats[m];
  for (size_t i = 0; m < n && i < ctx->dec_launches.size(); i++) out[m++] = ctx->dec_launches[i];
  return m;
}

int h9g_ordered_stats(h9g_ctx *ctx, int64_t *out, int n) {
  if (!ctx || !out || n < 1) return H9G_EINVAL;
  int m = 0;
  for (; m < n && m < 9; m++) out[m] = ctx->ord_stats[m];
  for (size_t i = 0; m < n && i < ctx->ord_passes.size(); i++) out[m++] = ctx->ord_passes[i];
  return m;
}

}  // extern "C"
