// h9g_stat.hip -- day statistics on the device (h9g_get_daystats,
// include/h9g.h): per cell and year the 17 annual indices of h9g_stat.h,
// reduced over the day axis of the day records where they lie (RecStream:
// d_year, or ret_year after an ordered call).  Host runtime (h9g_ctx.h) and
// its one kernel; instantiates no year kernel and changes no run path.
//
// h9g_daystat_kernel<W>: lane = cell, so every row read of a wave is 256
// contiguous bytes (the records are cell fastest).  A workgroup of W waves owns
// 64 cells, wave w the w-th contiguous slice of the year's days (stat_slice),
// blockIdx.y the year of the span.  A wave reads its slice in batches of seven
// days -- 49 independent loads issued before the first is used -- and keeps
// row 0 of the batch before (the seven S[d-7]) and rows 0 and 1 of the day
// before in registers; at the start of its slice it reads those from the days
// before the slice, which are another wave's days: further reads of the same
// rows, nothing is handed from wave to wave.  The W summaries of a cell go to
// LDS, wave 0 appends them in slice order (stat_merge) and stores the 17
// doubles, 64 neighbouring cells a row.  No atomic, no inter-workgroup
// protocol, no call; lanes past the last cell read the last cell's column and
// store nothing.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "h9g_ctx.h"
#include "h9g_stat.h"

using namespace h9k;

// The product's W (the fastest of those built on the 0.5 deg
// grid); H9G_DAYSTAT_W selects another of those built, for measurement.
#define H9G_STAT_W 8
#define H9G_STAT_WMAX 16
#define H9G_STAT_BATCH 7          // days a wave loads at once: the span of q7
#define H9G_STAT_YEARS 512        // years a launch's lengths are described for

struct StatArgs {
  const float *rec;      // the span's first year, (days, 7, n) at year_stride floats a year
  size_t year_stride;
  double *out;           // (years, 17, n)
  int n;
  int nseg;              // slices a year is cut into, 1 .. W
  int nt0;               // a year has nt0 days, or nt0 + 1 where its bit of `longer` is set
  unsigned longer[H9G_STAT_YEARS / 32];
  h9g_daystat_opts o;
};

template <int W>
__global__ void __launch_bounds__(W * 64) h9g_daystat_kernel(StatArgs a) {
  __shared__ DayStat sm[W > 1 ? W - 1 : 1][64];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const int y = (int)blockIdx.y;
  const int nt = a.nt0 + (int)((a.longer[y >> 5] >> (y & 31)) & 1u);
  const size_t n = (size_t)a.n;
  const size_t c = (size_t)blockIdx.x * 64 + (size_t)lane;
  const float *__restrict__ p = a.rec + (size_t)y * a.year_stride + (c < n ? c : n - 1);
  DayStat s;
  stat_init(s);
  if (w < a.nseg) {                                  // (wave-uniform)
    int lo, hi;
    stat_slice(nt, a.nseg, w, lo, hi);
    float ring[H9G_STAT_BATCH];                      // row 0 of days d-7 of the batch's days d
    double p0 = 0.0, p1 = 0.0;                       // rows 0 and 1 of the day before
    if (lo < hi) {
#pragma unroll
      for (int j = 0; j < H9G_STAT_BATCH; j++) {
        const int d = lo - H9G_STAT_BATCH + j;
        ring[j] = d >= 0 ? p[(size_t)d * STAT_NREC * n] : 0.0f;
      }
      if (lo > 0) {
        p0 = (double)p[((size_t)(lo - 1) * STAT_NREC + 0) * n];
        p1 = (double)p[((size_t)(lo - 1) * STAT_NREC + 1) * n];
      }
    }
    for (int d0 = lo; d0 < hi; d0 += H9G_STAT_BATCH) {
      float v[H9G_STAT_BATCH][STAT_NREC];
#pragma unroll
      for (int j = 0; j < H9G_STAT_BATCH; j++) {
        const int d = d0 + j < hi ? d0 + j : hi - 1;  // (a day past the slice: the slice's last again, not folded)
#pragma unroll
        for (int r = 0; r < STAT_NREC; r++) v[j][r] = p[((size_t)d * STAT_NREC + r) * n];
      }
#pragma unroll
      for (int j = 0; j < H9G_STAT_BATCH; j++) {
        if (d0 + j < hi) {
          stat_day(s, d0 + j, v[j], p0, (double)ring[j], p1, a.o);
          p0 = (double)v[j][0];
          p1 = (double)v[j][1];
          ring[j] = v[j][0];
        }
      }
    }
  }
  if (w > 0) sm[w - 1][lane] = s;
  __syncthreads();
  if (w == 0) {
    for (int k = 1; k < W; k++) {
      const DayStat b = sm[k - 1][lane];
      stat_merge(s, b);
    }
    double rows[H9G_NDAYSTAT];
    stat_rows(s, rows);
    if (c < n) {
      double *__restrict__ o = a.out + (size_t)y * H9G_NDAYSTAT * n + c;
#pragma unroll
      for (int r = 0; r < H9G_NDAYSTAT; r++) o[(size_t)r * n] = rows[r];
    }
  }
}

struct StatBufs {
  double *out = nullptr;          // the last call's result, (years, 17, n)
  size_t cap = 0;                 // doubles allocated there
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.0f;                // device time of the last call's launches
  int W = H9G_STAT_W;
};

static bool stat_w_built(int W) { return W == 4 || W == 8 || W == 16; }

// years [0, nk) of `a` through h9g_daystat_kernel<W>
static int stat_launch(int W, const StatArgs &a, int nk, hipStream_t stream) {
  const dim3 grid((unsigned)(((size_t)a.n + 63) / 64), (unsigned)nk);
  switch (W) {
    case 4: h9g_daystat_kernel<4><<<grid, 4 * 64, 0, stream>>>(a); break;
    case 8: h9g_daystat_kernel<8><<<grid, 8 * 64, 0, stream>>>(a); break;
    case 16: h9g_daystat_kernel<16><<<grid, 16 * 64, 0, stream>>>(a); break;
    default: return H9G_EINVAL;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Years of nt[0..nk) days each, nseg slices a year, into out: as many
// launches as it takes to describe the years' lengths (one, for calendar years).
static int stat_run(int W, int nseg, const float *rec, size_t year_stride, size_t n, const int *nt, int nk,
                    const h9g_daystat_opts *opts, double *out, hipStream_t stream) {
  for (int k = 0; k < nk;) {
    StatArgs a;
    memset(&a, 0, sizeof(a));
    a.rec = rec + (size_t)k * year_stride;
    a.year_stride = year_stride;
    a.out = out + (size_t)k * H9G_NDAYSTAT * n;
    a.n = (int)n;
    a.nseg = nseg;
    a.o = *opts;
    int lo = nt[k], hi = nt[k], m = 1;
    while (k + m < nk && m < H9G_STAT_YEARS) {
      const int v = nt[k + m], l2 = v < lo ? v : lo, h2 = v > hi ? v : hi;
      if (h2 - l2 > 1) break;
      lo = l2;
      hi = h2;
      m++;
    }
    a.nt0 = lo;
    for (int j = 0; j < m; j++)
      if (nt[k + j] > lo) a.longer[j >> 5] |= 1u << (j & 31);
    if (int r = stat_launch(W, a, m, stream)) return r;
    k += m;
  }
  return 0;
}

extern "C" {

void stat_free(h9g_ctx *ctx) {
  StatBufs *s = ctx->stat;
  if (!s) return;
  (void)hipFree(s->out);
  if (s->e0) (void)hipEventDestroy(s->e0);
  if (s->e1) (void)hipEventDestroy(s->e1);
  delete s;
  ctx->stat = nullptr;
}

int h9g_get_daystats(h9g_ctx *ctx, int k0, int nk, const h9g_daystat_opts *opts, double *out) {
  if (!ctx || !out || !stat_opts_ok(opts)) return H9G_EINVAL;
  const RecStream &rs = ctx->rec[REC_DAY];
  if (rs.nt.empty()) return H9G_ESTATE;
  if (k0 < 0 || nk < 1 || (size_t)k0 + (size_t)nk > rs.nt.size()) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = ctx->n, need = (size_t)nk * H9G_NDAYSTAT * n;
  if (!ctx->stat) {
    StatBufs *nb = new StatBufs();
    if (hipEventCreate(&nb->e0) != hipSuccess || hipEventCreate(&nb->e1) != hipSuccess) {
      (void)hipGetLastError();
      if (nb->e0) (void)hipEventDestroy(nb->e0);
      delete nb;
      return H9G_EHIP;
    }
    ctx->stat = nb;
  }
  StatBufs *s = ctx->stat;
  s->W = H9G_STAT_W;
  if (const char *e = getenv("H9G_DAYSTAT_W"))       // (measurement: another of the workgroups built)
    if (stat_w_built(atoi(e))) s->W = atoi(e);
  if (s->cap < need) {
    HIPCHK(hipStreamSynchronize(ctx->sc));
    (void)hipFree(s->out);
    s->out = nullptr;
    s->cap = 0;
    if (hipMalloc(&s->out, sizeof(double) * need) != hipSuccess) {
      (void)hipGetLastError();
      s->out = nullptr;
      return H9G_ENOMEM;
    }
    s->cap = need;
  }
  // the records where rec_get reads them: never copied
  const float *rec = rs.in_ret ? rs.ret_year(n, k0) : rs.d_year;
  HIPCHK(hipEventRecord(s->e0, ctx->sc));
  if (int r = stat_run(s->W, s->W, rec, rs.year_floats(n), n, rs.nt.data() + k0, nk, opts, s->out, ctx->sc)) return r;
  HIPCHK(hipEventRecord(s->e1, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipEventElapsedTime(&s->ms, s->e0, s->e1));
  HIPCHK(hipMemcpy(out, s->out, sizeof(double) * need, hipMemcpyDeviceToHost));
  return 0;
}

float h9g_last_daystat_ms(h9g_ctx *ctx) { return ctx && ctx->stat ? ctx->stat->ms : 0.0f; }

int h9g_daystat_selftest(int device, int n, int nt, int nseg, const float *records, const h9g_daystat_opts *opts,
                         double *out) {
  if (n < 1 || nt < 1 || nseg < 0 || nseg > H9G_STAT_WMAX || !records || !out || !stat_opts_ok(opts))
    return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  // nseg slices through the smallest kernel built with that many waves
  int W = H9G_STAT_W;
  if (nseg > 0) {
    W = 4;
    while (W < nseg) W *= 2;
  }
  const size_t nn = (size_t)n, floats = (size_t)nt * STAT_NREC * nn;
  float *d_rec = nullptr;
  double *d_out = nullptr;
  HIPCHK(hipMalloc(&d_rec, sizeof(float) * floats));
  if (hipMalloc(&d_out, sizeof(double) * H9G_NDAYSTAT * nn) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(d_rec);
    return H9G_ENOMEM;
  }
  int rc = 0;
  if (hipMemcpy(d_rec, records, sizeof(float) * floats, hipMemcpyHostToDevice) != hipSuccess) rc = H9G_EHIP;
  if (!rc) rc = stat_run(W, nseg > 0 ? nseg : W, d_rec, floats, nn, &nt, 1, opts, d_out, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = H9G_EHIP;
  if (!rc && hipMemcpy(out, d_out, sizeof(double) * H9G_NDAYSTAT * nn, hipMemcpyDeviceToHost) != hipSuccess)
    rc = H9G_EHIP;
  (void)hipFree(d_rec);
  (void)hipFree(d_out);
  return rc;
}

}  // extern "C"
