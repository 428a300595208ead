// h9g_quant.hip -- day quantiles on the device (h9g_get_dayquant,
// include/h9g.h): per cell, order statistics of one daily series over a year,
// or over all years of a span, selected from the day records where they lie
// (RecStream: d_year, or ret_year after an ordered call).  Host runtime
// (h9g_ctx.h) and its one kernel; instantiates no year kernel and changes no
// run path.
//
// h9g_dayquant_kernel<K, B, W, G>: lane = cell, so every row read of a wave is
// 256 contiguous bytes.  A workgroup of W waves owns 64 cells and one result
// (blockIdx.y: a year, or the pooled span); wave w reads the w-th slice of
// every year's days (quant_slice).  MSB-first radix selection on the monotone
// key K (h9g_quant.h), G ranks at once: a pass streams the series once and
// counts, per rank, the digit (B bits) of the candidates under the rank's
// prefix into the lane's own column of an LDS histogram (LDS adds: integer
// sums of the W waves, no order to matter); every wave then finds the rank's
// bin in the cell's column, so all hold the same prefixes and nothing is
// broadcast.  One last pass takes the smallest key above each rank's (LDS
// minimum): x_(j+1) where it is not x_(j) again.  The host launches the ranks
// in groups of G.  No global atomic, no inter-workgroup protocol, no call;
// lanes past the last cell read the last cell's column and store nothing.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "h9g_ctx.h"
#include "h9g_quant.h"

using namespace h9k;

// The product's variant (the fastest of those built on the 0.5
// deg grid); H9G_DAYQUANT_BITS / H9G_DAYQUANT_W select another of those built
// and H9G_DAYQUANT_KEY64 the 64-bit key for series 2..6 too, for measurement.
#define H9G_QUANT_BITS 4
#define H9G_QUANT_W 8
#define H9G_QUANT_WMAX 16
#define H9G_QUANT_BATCH 8          // days a wave loads at once
#define H9G_QUANT_YEARS 512        // years a launch's lengths are described for

// ranks a launch selects at once with digits of B bits (the histogram of a
// workgroup is G x 2^B x 64 counters: 16 KB, 16 KB and 64 KB)
constexpr int quant_group(int B) { return B == 8 ? 1 : 4; }

struct QuantArgs {
  const float *rec;      // the span's first year, (days, 7, n) at year_stride floats a year
  size_t year_stride;
  double *out;           // (results, 1 + 2 nq, n)
  int n;
  int nseg;              // slices a year is cut into, 1 .. W
  int nyears;            // years described in nt (pooled: the years of the one result)
  int r0, g;             // this launch's ranks: p[r0 .. r0+g)
  h9g_dayquant_opts o;
  uint16_t nt[H9G_QUANT_YEARS];   // days of each year
};

template <typename K, int B, int W, int G>
__global__ void __launch_bounds__(W * 64) h9g_dayquant_kernel(QuantArgs a) {
  using S = QuantShape<K, B>;
  static_assert(W >= G && G * S::NB * 4 >= G * (int)sizeof(K), "one array for the counters and the successors");
  __shared__ uint32_t sm[G * S::NB * 64];          // hist[r][digit][lane]; in the last pass succ[r][lane]
  K *const succ = (K *)sm;
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int y0 = a.o.pooled ? 0 : (int)blockIdx.y, y1 = a.o.pooled ? a.nyears : y0 + 1;
  const size_t n = (size_t)a.n, day = (size_t)QUANT_NREC * n;
  const size_t c = (size_t)blockIdx.x * 64 + (size_t)lane;
  const float *__restrict__ p = a.rec + (size_t)a.o.series * n + (c < n ? c : n - 1);
  const bool diff = quant_is_diff(a.o.series);
  QuantRank<K> rk[G];
  uint32_t jt[G];
  uint32_t m = 0;
#pragma unroll
  for (int r = 0; r < G; r++) {
    quant_init(rk[r]);
    jt[r] = 0;
  }
  for (int pass = 0; pass <= S::NP; pass++) {        // (pass NP: the successors)
    if (pass < S::NP) {
      for (int i = tid; i < G * S::NB * 64; i += W * 64) sm[i] = 0u;
    } else if (tid < G * 64) {
      succ[tid] = ~(K)0;
    }
    __syncthreads();
    if (w < a.nseg) {                                // (wave-uniform)
      for (int y = y0; y < y1; y++) {
        int lo, hi;
        quant_slice((int)a.nt[y], a.nseg, w, lo, hi);
        const float *__restrict__ py = p + (size_t)y * a.year_stride;
        float prev = diff && lo > 0 && lo < hi ? py[(size_t)(lo - 1) * day] : 0.0f;
        for (int d0 = lo; d0 < hi; d0 += H9G_QUANT_BATCH) {
          float v[H9G_QUANT_BATCH];
#pragma unroll
          for (int j = 0; j < H9G_QUANT_BATCH; j++) {
            const int d = d0 + j < hi ? d0 + j : hi - 1;   // (a day past the slice: the slice's last again, not counted)
            v[j] = py[(size_t)d * day];
          }
#pragma unroll
          for (int j = 0; j < H9G_QUANT_BATCH; j++) {
            if (d0 + j < hi) {
              K key;
              const bool ok = quant_cand(diff, v[j], prev, key);
              prev = v[j];
              if (ok) {
#pragma unroll
                for (int r = 0; r < G; r++) {
                  if (r < a.g) {
                    if (pass < S::NP) {
                      int dg;
                      if (quant_digit<K, B>(key, rk[r].prefix, pass, dg)) atomicAdd(&sm[(r * S::NB + dg) * 64 + lane], 1u);
                    } else if (key > rk[r].prefix) {
                      atomicMin(&succ[r * 64 + lane], key);
                    }
                  }
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    if (pass < S::NP) {
#pragma unroll
      for (int r = 0; r < G; r++) {
        if (r < a.g) {
          if (pass == 0) {
            uint32_t t = 0;
            for (int b = 0; b < S::NB; b++) t += sm[(r * S::NB + b) * 64 + lane];
            m = t;                                   // (every rank counted every candidate)
            jt[r] = m ? quant_target(a.o.p[a.r0 + r], m) : 0u;
            rk[r].rem = jt[r];
          }
          quant_step<K, B>(rk[r], [&](int b) { return sm[(r * S::NB + b) * 64 + lane]; });
        }
      }
    } else if (w == 0 && c < n) {
      const size_t rows = (size_t)(1 + 2 * a.o.nq);
      double *__restrict__ o = a.out + (size_t)blockIdx.y * rows * n + c;
      o[0] = (double)m;
#pragma unroll
      for (int r = 0; r < G; r++) {
        if (r < a.g) {
          const double x = m ? quant_value(rk[r].prefix) : __builtin_nan("");
          const double x1 = quant_needs_succ(rk[r], jt[r], m) ? quant_value(succ[r * 64 + lane]) : x;
          o[(size_t)(1 + 2 * (a.r0 + r)) * n] = x;
          o[(size_t)(2 + 2 * (a.r0 + r)) * n] = x1;
        }
      }
    }
    __syncthreads();
  }
}

struct QuantBufs {
  double *out = nullptr;          // the last call's result, (results, 1 + 2 nq, n)
  size_t cap = 0;                 // doubles allocated there
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.0f;                // device time of the last call's launches
};

struct QuantVariant {
  int B = H9G_QUANT_BITS, W = H9G_QUANT_W, key64 = 0;
};

// The variant the environment asks for, among those built.
static QuantVariant quant_variant() {
  QuantVariant v;
  if (const char *e = getenv("H9G_DAYQUANT_BITS")) {
    const int b = atoi(e);
    if (b == 2 || b == 4 || b == 8) v.B = b;
  }
  if (const char *e = getenv("H9G_DAYQUANT_W")) {
    const int w = atoi(e);
    if (w == 4 || w == 8 || w == 16) v.W = w;
  }
  if (const char *e = getenv("H9G_DAYQUANT_KEY64")) v.key64 = atoi(e) != 0;
  return v;
}

template <typename K, int B>
static int quant_launch_w(int W, const QuantArgs &a, dim3 grid, hipStream_t stream) {
  constexpr int G = quant_group(B);
  switch (W) {
    case 4: h9g_dayquant_kernel<K, B, 4, G><<<grid, 4 * 64, 0, stream>>>(a); break;
    case 8: h9g_dayquant_kernel<K, B, 8, G><<<grid, 8 * 64, 0, stream>>>(a); break;
    case 16: h9g_dayquant_kernel<K, B, 16, G><<<grid, 16 * 64, 0, stream>>>(a); break;
    default: return H9G_EINVAL;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

template <typename K>
static int quant_launch_b(const QuantVariant &v, const QuantArgs &a, dim3 grid, hipStream_t stream) {
  switch (v.B) {
    case 2: return quant_launch_w<K, 2>(v.W, a, grid, stream);
    case 4: return quant_launch_w<K, 4>(v.W, a, grid, stream);
    case 8: return quant_launch_w<K, 8>(v.W, a, grid, stream);
    default: return H9G_EINVAL;
  }
}

// Years of nt[0..nk) days each, nseg slices a year, into out: the ranks in
// groups of quant_group(B); per year, as many launches as it takes to describe
// the years' lengths (one up to H9G_QUANT_YEARS years).
static int quant_run(const QuantVariant &v, int nseg, const float *rec, size_t year_stride, size_t n, const int *nt,
                     int nk, const h9g_dayquant_opts *opts, double *out, hipStream_t stream) {
  if (opts->pooled && nk > H9G_QUANT_YEARS) return H9G_EINVAL;
  const bool key64 = v.key64 || quant_is_diff(opts->series);
  const int G = quant_group(v.B);
  const size_t rows = (size_t)(1 + 2 * opts->nq);
  for (int k = 0; k < nk;) {
    const int m = nk - k < H9G_QUANT_YEARS ? nk - k : H9G_QUANT_YEARS;
    QuantArgs a;
    memset(&a, 0, sizeof(a));
    a.rec = rec + (size_t)k * year_stride;
    a.year_stride = year_stride;
    a.out = out + (size_t)k * rows * n;
    a.n = (int)n;
    a.nseg = nseg;
    a.nyears = m;
    a.o = *opts;
    for (int j = 0; j < m; j++) a.nt[j] = (uint16_t)nt[k + j];
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)(opts->pooled ? 1 : m));
    for (int r0 = 0; r0 < opts->nq; r0 += G) {
      a.r0 = r0;
      a.g = opts->nq - r0 < G ? opts->nq - r0 : G;
      const int rc = key64 ? quant_launch_b<uint64_t>(v, a, grid, stream) : quant_launch_b<uint32_t>(v, a, grid, stream);
      if (rc) return rc;
    }
    k += m;
  }
  return 0;
}

extern "C" {

void quant_free(h9g_ctx *ctx) {
  QuantBufs *s = ctx->quant;
  if (!s) return;
  (void)hipFree(s->out);
  if (s->e0) (void)hipEventDestroy(s->e0);
  if (s->e1) (void)hipEventDestroy(s->e1);
  delete s;
  ctx->quant = nullptr;
}

int h9g_get_dayquant(h9g_ctx *ctx, int k0, int nk, const h9g_dayquant_opts *opts, double *out) {
  if (!ctx || !out || !quant_opts_ok(opts)) return H9G_EINVAL;
  const RecStream &rs = ctx->rec[REC_DAY];
  if (rs.nt.empty()) return H9G_ESTATE;
  if (k0 < 0 || nk < 1 || (size_t)k0 + (size_t)nk > rs.nt.size()) return H9G_EINVAL;
  if (opts->pooled && nk > H9G_QUANT_YEARS) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = ctx->n, need = (size_t)(opts->pooled ? 1 : nk) * (size_t)(1 + 2 * opts->nq) * n;
  if (!ctx->quant) {
    QuantBufs *nb = new QuantBufs();
    if (hipEventCreate(&nb->e0) != hipSuccess || hipEventCreate(&nb->e1) != hipSuccess) {
      (void)hipGetLastError();
      if (nb->e0) (void)hipEventDestroy(nb->e0);
      delete nb;
      return H9G_EHIP;
    }
    ctx->quant = nb;
  }
  QuantBufs *s = ctx->quant;
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
  const QuantVariant v = quant_variant();
  HIPCHK(hipEventRecord(s->e0, ctx->sc));
  if (int r = quant_run(v, v.W, rec, rs.year_floats(n), n, rs.nt.data() + k0, nk, opts, s->out, ctx->sc)) return r;
  HIPCHK(hipEventRecord(s->e1, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipEventElapsedTime(&s->ms, s->e0, s->e1));
  HIPCHK(hipMemcpy(out, s->out, sizeof(double) * need, hipMemcpyDeviceToHost));
  return 0;
}

float h9g_last_dayquant_ms(h9g_ctx *ctx) { return ctx && ctx->quant ? ctx->quant->ms : 0.0f; }

int h9g_dayquant_selftest(int device, int n, int nyears, const int32_t *nt, int nseg, const float *records,
                          const h9g_dayquant_opts *opts, double *out) {
  if (n < 1 || nyears < 1 || nyears > H9G_QUANT_YEARS || !nt || nseg < 0 || nseg > H9G_QUANT_WMAX || !records ||
      !out || !quant_opts_ok(opts))
    return H9G_EINVAL;
  int ntmax = 0;
  for (int y = 0; y < nyears; y++) {
    if (nt[y] < 1 || nt[y] > 65535) return H9G_EINVAL;
    if (nt[y] > ntmax) ntmax = nt[y];
  }
  HIPCHK(hipSetDevice(device));
  // nseg slices through the smallest workgroup built with that many waves
  QuantVariant v = quant_variant();
  if (nseg > 0) {
    v.W = 4;
    while (v.W < nseg) v.W *= 2;
  }
  const size_t nn = (size_t)n, year = (size_t)ntmax * QUANT_NREC * nn, floats = (size_t)nyears * year;
  const size_t doubles = (size_t)(opts->pooled ? 1 : nyears) * (size_t)(1 + 2 * opts->nq) * nn;
  float *d_rec = nullptr;
  double *d_out = nullptr;
  HIPCHK(hipMalloc(&d_rec, sizeof(float) * floats));
  if (hipMalloc(&d_out, sizeof(double) * doubles) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(d_rec);
    return H9G_ENOMEM;
  }
  int rc = 0;
  if (hipMemcpy(d_rec, records, sizeof(float) * floats, hipMemcpyHostToDevice) != hipSuccess) rc = H9G_EHIP;
  if (!rc) rc = quant_run(v, nseg > 0 ? nseg : v.W, d_rec, year, nn, nt, nyears, opts, d_out, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = H9G_EHIP;
  if (!rc && hipMemcpy(out, d_out, sizeof(double) * doubles, hipMemcpyDeviceToHost) != hipSuccess) rc = H9G_EHIP;
  (void)hipFree(d_rec);
  (void)hipFree(d_out);
  return rc;
}

}  // extern "C"
