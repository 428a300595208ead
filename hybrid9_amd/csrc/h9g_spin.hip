// h9g_spin.hip -- spin-up to equilibrium (h9g_spinup, include/h9g.h): a
// forcing period repeated on the device, every cell tested after each cycle
// against its own state one cycle earlier, settled cells retired.  Host
// runtime (h9g_ctx.h); instantiates no year kernel.
//
// The years are run_year_impl's launches, untouched: an every-cell launch as
// h9g_run_year makes it while no cell has left, a list launch of the active
// cells on the context's own state afterwards (the kernel by the list's
// length, list_kind).  Isolated cells are independent -- each carries its own
// smp -- so leaving a cell out changes no other cell's bits.
//
// h9g_spin_kernel, once per cycle: one workgroup of 1,024 threads over the
// cells in chunks of 1,024 (the shape of h9g_diag_kernel: it runs once per
// cycle of at least one grid year, over a few hundred kilobytes; one
// workgroup needs no inter-block protocol and no atomic).  Per cell the test
// of h9g_spin.h; the next cycle's list by an ordered compaction -- a 64-bit
// ballot and the count of the lanes below within a wave, a scan of the 16
// waves' counts in LDS, a running base over the chunks -- so the list is
// strictly increasing and two runs make identical launches.  The maxima are
// exact whatever the order.  The host reads the counters block (eight
// doubles) once per cycle: it needs the list's length to size the next launch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <vector>

#include "h9g_ctx.h"
#include "h9g_spin.h"

#define H9G_SPIN_THREADS 1024
#define H9G_SPIN_WAVES (H9G_SPIN_THREADS / 64)
#define H9G_SPIN_NSTAT 8   // the history row, the list's length, cells that can run at all

struct SpinArgs {
  int n, L;
  int k;        // the cycle tested; 0: the call's start (keys of cycle 0, who can run, the first list)
  int freeze;
  int jyear;    // the cycle's last year (a STOP not marked yet happened in it)
  SpinTol tol;
  const float *st;     // state rows of n
  const float *par;    // parameter rows of n (k = 0: the soil mask; null: no cell masked)
  const int *err;      // STOP rows of n (null: no cell stopped)
  double *keys;        // SPIN_KEYS rows of n: W, zwt, pm one cycle earlier
  int *cc;             // cell_cycle
  int *sy;             // year of a cell's STOP in this call (0: none; may be null)
  int *list;           // out: the cells still active, increasing
  double *stats;       // out: H9G_SPIN_NSTAT
};

struct SpinBufs {
  double *keys = nullptr, *stats = nullptr;
  int *cc = nullptr, *sy = nullptr, *list = nullptr;
};

// A cell of the call that has a STOP record and no year yet stopped in `jyear`.
__device__ __forceinline__ void spin_mark(int c, int jyear, const int *err, const int *cc, int *sy) {
  if (cc[c] >= SPIN_ACTIVE && err[c] != 0 && sy[c] == 0) sy[c] = jyear;
}

// After a year of a cycle that is not its last (the last year's: h9g_spin_kernel).
__global__ void __launch_bounds__(256) h9g_spin_mark_kernel(int n, int jyear, const int *__restrict__ err,
                                                            const int *__restrict__ cc, int *__restrict__ sy) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) spin_mark(c, jyear, err, cc, sy);
}

__global__ void __launch_bounds__(H9G_SPIN_THREADS) h9g_spin_kernel(SpinArgs a) {
  __shared__ int wcount[H9G_SPIN_WAVES];
  __shared__ double red[H9G_SPIN_THREADS];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = (size_t)a.n;
  int base = 0;                                   // the list's length so far (the same in every thread)
  double cnt[3] = {0.0, 0.0, 0.0};                // cells run, settled, stopped
  double dmax[3] = {0.0, 0.0, 0.0};               // maxima of d_w, d_z, d_p
  for (int c0 = 0; c0 < a.n; c0 += H9G_SPIN_THREADS) {
    const int c = c0 + tid;
    bool active = false;
    if (c < a.n) {
      if (a.k == 0) {
        const bool runs = (!a.par || spin_soil(a.par, n, (size_t)c, a.L)) && (!a.err || a.err[c] == 0);
        a.cc[c] = runs ? SPIN_ACTIVE : SPIN_NEVER;
        if (a.sy) a.sy[c] = 0;
        if (runs) {
          const SpinKey key = spin_key(a.st, n, (size_t)c, a.L);
          a.keys[0 * n + c] = key.w;
          a.keys[1 * n + c] = key.zwt;
          a.keys[2 * n + c] = key.pm;
          cnt[0] += 1.0;
          active = true;
        }
      } else {
        const int cc = a.cc[c];
        if (a.freeze ? cc == SPIN_ACTIVE : cc >= SPIN_ACTIVE) {     // it ran this cycle
          cnt[0] += 1.0;
          if (a.err && a.err[c] != 0) {
            if (a.sy) spin_mark(c, a.jyear, a.err, a.cc, a.sy);
            a.cc[c] = SPIN_STOPPED;
            cnt[2] += 1.0;
          } else {
            const SpinKey prev = {a.keys[0 * n + c], a.keys[1 * n + c], a.keys[2 * n + c]};
            const SpinKey key = spin_key(a.st, n, (size_t)c, a.L);
            const SpinKey d = spin_drift(prev, key);
            dmax[0] = spin_max(dmax[0], d.w);
            dmax[1] = spin_max(dmax[1], d.zwt);
            dmax[2] = spin_max(dmax[2], d.pm);
            a.keys[0 * n + c] = key.w;
            a.keys[1 * n + c] = key.zwt;
            a.keys[2 * n + c] = key.pm;
            const bool met = spin_settled(d, a.k, a.tol);
            if (met && cc == SPIN_ACTIVE) {
              a.cc[c] = a.k;
              cnt[1] += 1.0;
            }
            active = !met;
          }
        }
      }
    }
    // ordered compaction of the chunk's active cells behind `base`
    const unsigned long long mask = __ballot(active);
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int below = 0, total = 0;
    for (int w = 0; w < H9G_SPIN_WAVES; w++) {
      const int v = wcount[w];
      below += w < wave ? v : 0;
      total += v;
    }
    if (active) a.list[base + below + __popcll(mask & ((1ull << lane) - 1ull))] = c;
    base += total;
    __syncthreads();                              // (wcount is the next chunk's too)
  }
  for (int j = 0; j < 6; j++) {
    red[tid] = j < 3 ? cnt[j] : dmax[j - 3];
    __syncthreads();
    for (int w = H9G_SPIN_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) red[tid] = j < 3 ? red[tid] + red[tid + w] : spin_max(red[tid], red[tid + w]);
      __syncthreads();
    }
    if (tid == 0) a.stats[j] = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    a.stats[6] = (double)base;
    a.stats[7] = 0.0;
  }
}

static bool spin_opts_ok(const h9g_spinup_opts *o) {
  return o && o->max_cycles >= 1 && o->min_cycles >= 1 && o->min_cycles <= o->max_cycles &&
         (o->freeze == 0 || o->freeze == 1) && o->reserved == 0 && o->tol_water >= 0.0 && o->tol_zwt >= 0.0 &&
         o->tol_plant >= 0.0;   // (false for a NaN)
}

static SpinTol spin_tol(const h9g_spinup_opts *o) { return {o->min_cycles, o->tol_water, o->tol_zwt, o->tol_plant}; }

extern "C" {

void spin_free(h9g_ctx *ctx) {
  SpinBufs *s = ctx->spin;
  if (!s) return;
  (void)hipFree(s->keys);
  (void)hipFree(s->stats);
  (void)hipFree(s->cc);
  (void)hipFree(s->sy);
  (void)hipFree(s->list);
  delete s;
  ctx->spin = nullptr;
}

static int spin_alloc(h9g_ctx *ctx) {
  if (ctx->spin) return 0;
  SpinBufs *s = ctx->spin = new SpinBufs();
  const size_t n = ctx->n;
  if (hipMalloc(&s->keys, sizeof(double) * SPIN_KEYS * n) != hipSuccess ||
      hipMalloc(&s->stats, sizeof(double) * H9G_SPIN_NSTAT) != hipSuccess ||
      hipMalloc(&s->cc, sizeof(int) * n) != hipSuccess || hipMalloc(&s->sy, sizeof(int) * n) != hipSuccess ||
      hipMalloc(&s->list, sizeof(int) * n) != hipSuccess) {
    (void)hipGetLastError();
    spin_free(ctx);
    return H9G_ENOMEM;
  }
  return 0;
}

// The test of cycle k (0: the call's start) on the compute stream, and its
// counters on the host (synchronises).
static int spin_test(h9g_ctx *ctx, const h9g_spinup_opts *opts, int k, int jyear, double *stats) {
  const SpinBufs *s = ctx->spin;
  SpinArgs a;
  a.n = (int)ctx->n;
  a.L = ctx->L;
  a.k = k;
  a.freeze = opts->freeze;
  a.jyear = jyear;
  a.tol = spin_tol(opts);
  a.st = ctx->d_st;
  a.par = ctx->d_par;
  a.err = ctx->d_err;
  a.keys = s->keys;
  a.cc = s->cc;
  a.sy = s->sy;
  a.list = s->list;
  a.stats = s->stats;
  h9g_spin_kernel<<<1, H9G_SPIN_THREADS, 0, ctx->sc>>>(a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(stats, s->stats, sizeof(double) * H9G_SPIN_NSTAT, hipMemcpyDeviceToHost));
  return 0;
}

int h9g_spinup(h9g_ctx *ctx, const int32_t *slots, int jyear0, int nyears, const h9g_spinup_opts *opts,
               int32_t *cycles_run, int32_t *cell_cycle, double *history) {
  if (!ctx || !slots || !spin_opts_ok(opts)) return H9G_EINVAL;
  if (nyears < 1 || nyears > ctx->cfg.nslots || jyear0 < 1861 || jyear0 + nyears - 1 > 2299) return H9G_EINVAL;
  {
    std::vector<char> used((size_t)ctx->cfg.nslots, 0);
    for (int y = 0; y < nyears; y++)
      if (slots[y] < 0 || slots[y] >= ctx->cfg.nslots || used[(size_t)slots[y]]++) return H9G_EINVAL;
  }
  if (!ctx->daily_sel.empty() || ctx->recording()) return H9G_ESTATE;   // spin-up records nothing
  if (!ctx->params_set || !ctx->state_set) return H9G_ESTATE;
  for (int y = 0; y < nyears; y++) {
    if (const int prc = join_prefetch(ctx, slots[y])) return prc;
    if (ctx->slot_days[(size_t)slots[y]] < days_in_year(jyear0 + y)) return H9G_EINVAL;
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (int r = spin_alloc(ctx)) return r;
  const size_t n = ctx->n;
  const SpinBufs *s = ctx->spin;
  if (cycles_run) *cycles_run = 0;
  if (history) memset(history, 0, sizeof(double) * (size_t)opts->max_cycles * H9G_NSPIN);
  double stats[H9G_SPIN_NSTAT];
  if (int r = spin_test(ctx, opts, 0, jyear0, stats)) return r;
  int m = (int)stats[6];     // the active cells (s->list)
  bool left = false;         // a cell has left the run: the years are list launches from here on
  for (int k = 1; k <= opts->max_cycles && m > 0; k++) {
    for (int y = 0; y < nyears; y++) {
      YearSpec ys;
      ys.slot = slots[y];
      ys.jyear = jyear0 + y;
      if (left) {
        ys.d_list = s->list;
        ys.m = m;
        ys.ann_dst = ctx->d_ann;
      }
      if (int r = run_year_impl(ctx, ys)) return r;
      if (y < nyears - 1) {
        h9g_spin_mark_kernel<<<nblocks(n), H9G_BLOCK, 0, ctx->sc>>>((int)n, jyear0 + y, ctx->d_err, s->cc, s->sy);
        HIPCHK(hipGetLastError());
      }
    }
    if (int r = spin_test(ctx, opts, k, jyear0 + nyears - 1, stats)) return r;
    if (history) memcpy(history + (size_t)(k - 1) * H9G_NSPIN, stats, sizeof(double) * H9G_NSPIN);
    if (cycles_run) *cycles_run = k;
    m = (int)stats[6];
    if (opts->freeze && (stats[1] > 0.0 || stats[2] > 0.0)) left = true;
  }
  // the diagnostics over the rows the call leaves (a list launch computes none)
  if (int r = diag_launch(ctx)) return r;
  std::vector<int> cc(n);
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(cc.data(), s->cc, sizeof(int) * n, hipMemcpyDeviceToHost));
  if (cell_cycle) memcpy(cell_cycle, cc.data(), sizeof(int) * n);
  if (ctx->last_err.code == 0) {
    // the first cell in context order to STOP in this call, with its year
    for (size_t c = 0; c < n; c++) {
      if (cc[c] != SPIN_STOPPED) continue;
      int e[STOP_ROWS], year = 0;
      for (int r = 0; r < STOP_ROWS; r++)
        HIPCHK(hipMemcpy(&e[r], ctx->d_err + (size_t)r * n + c, sizeof(int), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&year, s->sy + c, sizeof(int), hipMemcpyDeviceToHost));
      bool earlier = false;    // (a STOP from before the call that no h9g_sync has reported comes first)
      std::vector<int> code(c);
      if (c > 0) HIPCHK(hipMemcpy(code.data(), ctx->d_err, sizeof(int) * c, hipMemcpyDeviceToHost));
      for (size_t b = 0; b < c; b++) earlier |= code[b] != 0;
      if (!earlier) {
        ctx->last_err.code = e[0];
        ctx->last_err.cell = (int)c;
        ctx->last_err.year = year;
        ctx->last_err.day = e[1];
        ctx->last_err.substep = e[2];
        ctx->last_err.value = __builtin_bit_cast(float, e[3]);
      }
      break;
    }
  }
  return h9g_sync(ctx);
}

int h9g_spin_selftest(int device, int n, int L, const float *state_prev, const float *state, const int32_t *err,
                      const h9g_spinup_opts *opts, int k, int32_t *list, int32_t *cell_cycle, double *stats) {
  if (n <= 0 || (L != 8 && L != 10) || !state_prev || !state || !spin_opts_ok(opts) || k < 1 || !list ||
      !cell_cycle || !stats)
    return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  const size_t nn = (size_t)n, srows = (size_t)state_rows(L);
  std::vector<float> rows(2 * srows * nn);
  state_rows_from_packed(L, nn, state_prev, rows.data());
  state_rows_from_packed(L, nn, state, rows.data() + srows * nn);
  float *d_st = nullptr;
  double *d_keys = nullptr, *d_stats = nullptr;
  int *d_i = nullptr;      // rows of n: STOP codes, cell_cycle, list
  HIPCHK(hipMalloc(&d_st, sizeof(float) * rows.size()));
  HIPCHK(hipMalloc(&d_keys, sizeof(double) * SPIN_KEYS * nn));
  HIPCHK(hipMalloc(&d_stats, sizeof(double) * H9G_SPIN_NSTAT));
  HIPCHK(hipMalloc(&d_i, sizeof(int) * 3 * nn));
  HIPCHK(hipMemcpy(d_st, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice));
  if (err) HIPCHK(hipMemcpy(d_i, err, sizeof(int) * nn, hipMemcpyHostToDevice));
  SpinArgs a;
  a.n = n;
  a.L = L;
  a.k = 0;
  a.freeze = opts->freeze;
  a.jyear = 0;
  a.tol = spin_tol(opts);
  a.st = d_st;
  a.par = nullptr;
  a.err = nullptr;
  a.keys = d_keys;
  a.cc = d_i + nn;
  a.sy = nullptr;
  a.list = d_i + 2 * nn;
  a.stats = d_stats;
  h9g_spin_kernel<<<1, H9G_SPIN_THREADS>>>(a);
  HIPCHK(hipGetLastError());
  a.k = k;
  a.st = d_st + srows * nn;
  a.err = err ? d_i : nullptr;
  h9g_spin_kernel<<<1, H9G_SPIN_THREADS>>>(a);
  HIPCHK(hipGetLastError());
  double hs[H9G_SPIN_NSTAT];
  HIPCHK(hipMemcpy(hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost));
  memcpy(stats, hs, sizeof(double) * (H9G_NSPIN + 1));
  HIPCHK(hipMemcpy(cell_cycle, d_i + nn, sizeof(int) * nn, hipMemcpyDeviceToHost));
  const size_t m = (size_t)hs[6];
  if (m > 0) HIPCHK(hipMemcpy(list, d_i + 2 * nn, sizeof(int) * m, hipMemcpyDeviceToHost));
  (void)hipFree(d_st);
  (void)hipFree(d_keys);
  (void)hipFree(d_stats);
  (void)hipFree(d_i);
  return 0;
}

}  // extern "C"
