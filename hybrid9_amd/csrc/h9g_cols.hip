// h9g_cols.hip -- the one-lane-per-column kernels' translation unit: the four
// geometry-templated kernels beside the year kernels -- the initial state
// (h9g_init_kernel), the cell order of a year launch (h9g_sort_kernel), the
// LCLIM single-site run (h9g_site_kernel) and the daily diagnostics' shadow
// run (h9g_focus_kernel) -- each behind a launcher of h9g_year.h that picks
// the configuration's geometry variant and the grid.  A unit of its own so
// that no change to the host runtime compiles them again.
#include "h9g_year.h"

// Cell order of the next year kernel: a stable counting sort of the cells
// by where their water table was over the last year, failed cells last.
// Cells are independent, so the order changes no result; it makes the 22
// columns of a wave take the same branches that depend on the layer holding
// the water table (jwt, HYDROLOGY.f90:499-508): the equilibrium-profile cases
// (:517-567), the aquifer node (:574-590, :737-741) for jwt = L, the recharge
// (:856-904) and the water-table and drainage loops (:923-1118) for jwt < L.
// A wave holding both kinds of column runs both.  Keys:
//   0 .. L-1   no substep of the last year below the column: the current jwt
//   L .. L+7   some: the fraction of the year's substeps below it, in eighths
//   L+8        every substep below the column
//   L+9        failed
// Without a last year (hist < 0) the current jwt decides (jwt = L: key L+8).
// Round 2 sorted by the current jwt alone; cells whose water table crosses
// the column's bottom during the year then sat in waves of both kinds
// (measured with H9G_COUNT_BRANCH at 1906-1907: 84% of the wave-substeps ran
// the aquifer node, 81% the recharge).  Block x sorts the slots of XCD x's
// workgroups of the year launch over [c0, cend) with cpb cells per workgroup
// (xcd_vwg), so no cell leaves its XCD's range.  list (may be null): the
// slots hold the cells list[c0 .. cend) instead of c0 .. cend (the cell
// order's re-run lists; round 6).
#define H9G_SORT_THREADS 512
template <int L, class G>
__global__ void __launch_bounds__(H9G_SORT_THREADS)
    h9g_sort_kernel(int n, int c0, int cend, int cpb, const float *__restrict__ st, const int *__restrict__ err,
                    const int *__restrict__ hist, int nsub, int *__restrict__ perm, const int *__restrict__ list,
                    const G g) {
  constexpr int NK = L + 10;
  constexpr int NTH = H9G_SORT_THREADS;
  __shared__ int cnt[NK][NTH];
  __shared__ int base[NK];
  const int t = threadIdx.x;
  const unsigned nb = (unsigned)((cend - c0 + cpb - 1) / cpb), x = blockIdx.x;
  const unsigned q = nb / H9G_NXCD, r = nb % H9G_NXCD;
  const int p0 = c0 + (int)(x * q + (x < r ? x : r)) * cpb;
  const int p1 = min(cend, p0 + (int)(q + (x < r ? 1u : 0u)) * cpb);
  const int m = p1 - p0;
  if (m <= 0) return;                      // (uniform per block)
  const int per = (m + NTH - 1) / NTH;
  const int b = p0 + t * per, e = min(p1, b + per);
  float zim[L + 1];
#pragma unroll
  for (int i = 1; i <= L; i++) zim[i] = g.zim(i);
  const float *zwt = st + (size_t)scalar_row(L, SC_ZWT) * n;
  auto key = [&](int c) -> int {
    if (err[c]) return L + 9;
    const int j = jwt_of<L>(zwt[c], zim);
    const int h = hist ? hist[c] : -1;
    if (h < 0 || nsub <= 0) return j < L ? j : L + 8;
    if (h == 0) return j < L ? j : L;
    if (h >= nsub) return L + 8;
    return L + (int)((long long)h * 8 / nsub);
  };
  int loc[NK];
#pragma unroll
  for (int k = 0; k < NK; k++) loc[k] = 0;
  for (int c = b; c < e; c++) {
    const int k = key(list ? list[c] : c);
#pragma unroll
    for (int j = 0; j < NK; j++) loc[j] += (j == k);
  }
#pragma unroll
  for (int k = 0; k < NK; k++) cnt[k][t] = loc[k];
  __syncthreads();
  if (t < NK) {                   // exclusive scan of each key's counts over the threads
    int sum = 0;
    for (int j = 0; j < NTH; j++) {
      const int v = cnt[t][j];
      cnt[t][j] = sum;
      sum += v;
    }
    base[t] = sum;
  }
  __syncthreads();
  if (t == 0) {
    int sum = 0;
    for (int k = 0; k < NK; k++) {
      const int v = base[k];
      base[k] = sum;
      sum += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NK; k++) loc[k] = base[k] + cnt[k][t];
  for (int c = b; c < e; c++) {
    const int cell = list ? list[c] : c;
    const int k = key(cell);
    int pos = 0;
#pragma unroll
    for (int j = 0; j < NK; j++)
      if (j == k) pos = loc[j]++;
    perm[p0 + pos] = cell;
  }
}

// LCLIM single-site kernel (HYBRID9.f90:339-480): one lane per site,
// cell_site of h9g_pair.h.  Parameters and state as the year kernels.
template <int L, class G>
__global__ void __launch_bounds__(64) h9g_site_kernel(const SiteArgs a, const G g) {
  typedef SoloStore<L> SS;
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  __shared__ float s_cell[SS::ROWS * 64];
  __shared__ float s_zt[zt_size<L>()];
  if (threadIdx.x == 0) fill_zt<L>(g, s_zt);
  load_tabs(s_e2, s_l2);
  const h9m::Tabs T = {s_e2, s_l2};
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.ncell) return;
  const int n = a.ncell;
  SS cs{(lds_float *)&s_cell[threadIdx.x], (const lds_float *)s_zt};
  St<L> s;
  H9K_LOAD_LANE(L, cs, s, a.par, n, c, a.st, n, c)
  const float h2o_ma1 = a.st[(size_t)Rows<L>::H2O_MA * n + c];
  H9K_LOAD_SCALARS(L, s, a.st, n, c)
  H9K_TS_SUM(L, cs, ts_sum)
  if (!(ts_sum > SOIL_TRUNC) || a.err[c] != 0) {
    for (int d = 0; d < a.nday; d++) nan_rows(a.out + (size_t)d * DAILY_ROWS * n, DAILY_ROWS, n, c);
    return;
  }
  cell_inv_pair<L, G>(g, cs);
  int eday = 0, estep = 0;
  float errval = 0.0f;
  const int code = cell_site<L, G, SS>(g, cs, s, h2o_ma1, a.sub + c, a.daily + c, a.lai + c, a.out + c,
                                       (size_t)n, a.nday, a.nisurf, eday, estep, errval, T);
  H9K_STORE_CELL(L, s, cs, a.st, n, c, false, SC_SITE)
  if (code) {
    stop_write(a.err, n, c, code, eday, estep, errval, a.err_flag);
    for (int d = eday; d < a.nday; d++) nan_rows(a.out + (size_t)d * DAILY_ROWS * n, DAILY_ROWS, n, c);
  }
}

// Daily diagnostics of the selected cells (h9g_set_daily): the shadow run
// cell_focus of h9g_pair.h, one lane per selected cell.  It reads the cells'
// start state from a gathered copy (st: state rows of nsel, selection order;
// h9g_focus_gather_kernel), their parameters and forcing by cell id from the
// context's arrays and the forcing slots' original layout, and writes only
// out (days of all years, 11, nsel).
template <int L, class G>
__global__ void __launch_bounds__(64) h9g_focus_kernel(const FocusArgs a, const G g) {
  typedef SoloStore<L> SS;
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  __shared__ float s_cell[SS::ROWS * 64];
  __shared__ float s_zt[zt_size<L>()];
  if (threadIdx.x == 0) fill_zt<L>(g, s_zt);
  load_tabs(s_e2, s_l2);
  const h9m::Tabs T = {s_e2, s_l2};
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.nsel) return;
  const int c = a.sel[j];
  const int n = a.ncell, m = a.nsel;
  SS cs{(lds_float *)&s_cell[threadIdx.x], (const lds_float *)s_zt};
  St<L> s;
  H9K_LOAD_LANE(L, cs, s, a.par, n, c, a.st, m, j)
  const float h2o_ma1 = a.st[(size_t)Rows<L>::H2O_MA * m + j];
  H9K_LOAD_SCALARS(L, s, a.st, m, j)
  s.naq = 0;
  H9K_TS_SUM(L, cs, ts_sum)
  if (!(ts_sum > SOIL_TRUNC) || a.err[c] != 0) {      // masked, or stopped before the run: no line at all
    size_t d = 0;
    for (int y = 0; y < a.nyears; y++)
      for (int k = 0; k < a.yrs[y].nt; k++, d++) nan_rows(a.out + d * DAILY_ROWS * m, DAILY_ROWS, m, j);
    return;
  }
  cell_inv_pair<L, G>(g, cs);
  cell_focus<L, G, SS>(g, cs, s, h2o_ma1, a.yrs, a.nyears, (size_t)c, (size_t)n, a.fvar, a.nisurf, a.grow_on,
                       a.out + j, (size_t)m, T);
}

// init_cell's rootr array as H9K_STORE_CELL reads a store's rootr rows
struct InitRoots {
  const float *r;
  __device__ __forceinline__ float lay(int, int i) const { return r[i]; }
};

template <int L, class G>
__global__ void __launch_bounds__(H9G_BLOCK) h9g_init_kernel(int ncell, const float *__restrict__ par,
                                                             float *__restrict__ st, const G g) {
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  load_tabs(s_e2, s_l2);
  MathExact me{{s_e2, s_l2}};
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const int n = ncell;
  float ts[L + 1];
  St<L> s;
  float h2o_ma[L + 1], rootr[L + 1];
#pragma unroll
  for (int i = 1; i <= L; i++) ts[i] = par[(size_t)par_row(L, PF_TS, i - 1) * n + c];
  init_cell<L, G, MathExact>(g, ts, s, rootr, h2o_ma, me);
  const InitRoots roots{rootr};
  H9K_STORE_CELL(L, s, roots, st, n, c, true, SC_N)
#pragma unroll
  for (int i = 1; i <= L; i++) st[(size_t)(Rows<L>::H2O_MA + i - 1) * n + c] = h2o_ma[i];
}

int h9g_init_launch(const h9g_config *cfg, hipStream_t stream, int ncell, const float *par, float *st) {
  const unsigned grid = (unsigned)(((size_t)ncell + H9G_BLOCK - 1) / H9G_BLOCK);
  return geo_dispatch(*cfg, [&](auto L, auto g) {
    h9g_init_kernel<L, decltype(g)><<<grid, H9G_BLOCK, 0, stream>>>(ncell, par, st, g);
    return 0;
  });
}

int h9g_sort_launch(const h9g_config *cfg, hipStream_t stream, int n, int c0, int cend, int cpb, const float *st,
                    const int *err, const int *hist, int nsub, int *perm, const int *list) {
  return geo_dispatch(*cfg, [&](auto L, auto g) {
    h9g_sort_kernel<L, decltype(g)><<<H9G_NXCD, H9G_SORT_THREADS, 0, stream>>>(n, c0, cend, cpb, st, err, hist, nsub,
                                                                               perm, list, g);
    return 0;
  });
}

int h9g_site_launch(const h9g_config *cfg, hipStream_t stream, const SiteArgs &a) {
  return geo_dispatch(*cfg, [&](auto L, auto g) {
    h9g_site_kernel<L, decltype(g)><<<(unsigned)((a.ncell + 63) / 64), 64, 0, stream>>>(a, g);
    return 0;
  });
}

int h9g_focus_launch(const h9g_config *cfg, hipStream_t stream, const FocusArgs &a) {
  return geo_dispatch(*cfg, [&](auto L, auto g) {
    h9g_focus_kernel<L, decltype(g)><<<(unsigned)((a.nsel + 63) / 64), 64, 0, stream>>>(a, g);
    return 0;
  });
}
