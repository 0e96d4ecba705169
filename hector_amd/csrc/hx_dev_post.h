// hx_dev_post.h -- what a user does with a finished ensemble, on the device: a per-member misfit
// of a recorded output against an observation series (hx_score_kernel), per-member metrics of a
// window (hx_metric_kernel), of a window of two series (hx_pair_metric_kernel), exact weighted
// quantiles over the members (hx_q_* kernels),
// weighted bin sums against fixed edges (hx_bin_kernel) and weighted moments with per-member
// predictors (hx_mom_* / hx_moments_kernel) -- and, ahead of a run, the per-member input tables
// built from mixes (hx_mseries_mix_kernel) and the gas pre-pass from recipes (hx_gas_mix_kernel).
// The reference has no counterpart: its
// hosts aggregate fetchvars() data frames in R.  Compiled for the GPU through hx_post.hip -- a
// translation unit of its own, so the year-loop kernels' code generation does not see it -- and
// for the host-emulation build through ensemble_post.cpp, the one file that may include this one
// there, itself compiled as the tail of ensemble_core.cpp in that build (score, metric, pair-metric, series and mix kernels only: the quantile, bin and
// moment kernels are cooperative -- LDS atomics, cross-lane -- and one lane at a time cannot run
// them).  The records and constants the host fills or reads, and the launchers' prototypes, are in
// hx_post_abi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hector_amd.h"   // hx_metric, HX_MET_*
#include "hx_post_abi.h"

// ===========================================================================
// Score: chi2[lane] = sum_i r_i^2, r_i = ((x(iy[i], lane) - base) - obs[i]) / sigma[i], evaluated
// in exactly this order in IEEE double without fused multiply-add, so that numpy reproduces it
// bit for bit under any lane order, kernel flavour or shard layout.  One lane per member, the
// [year][npad] rows read coalesced; nothing is exchanged between lanes.
//   b0 <= b1: base = the lane's own mean of x over the rows b0..b1 (summed in that order);
//   b0 > b1: no baseline.  obs[i] NaN: skipped.  sigma == nullptr: no division.
// ===========================================================================
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_score_kernel(const double *var, int n, int npad,
                                                       const int *iy, const double *obs,
                                                       const double *sigma, int nobs, int b0, int b1,
                                                       double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= n) return;
  const bool has_base = b0 <= b1;
  double base = 0.0;
  if (has_base) {
    double s = 0.0;
    for (int y = b0; y <= b1; ++y) s = s + var[(size_t)y * npad + lane];
    base = s / (double)(b1 - b0 + 1);
  }
  double chi = 0.0;
  for (int i = 0; i < nobs; ++i) {
    const double o = obs[i];
    if (o != o) continue;
    const double x = var[(size_t)iy[i] * npad + lane];
    double r = has_base ? (x - base) - o : x - o;
    if (sigma) r = r / sigma[i];
    const double r2 = r * r;
    chi = chi + r2;
  }
  out[lane] = chi;
}

hipError_t hx_launch_score(const double *var, int n, int npad, const int *iy, const double *obs,
                           const double *sigma, int nobs, int b0, int b1, double *out,
                           hipStream_t st) {
  hipLaunchKernelGGL(hx_score_kernel, dim3((n + 255) / 256), dim3(256), 0, st, var, n, npad, iy, obs,
                     sigma, nobs, b0, b1, out);
  return hipGetLastError();
}

// ===========================================================================
// Metrics: one double per member from a window of a recorded output (hx_member_metrics in
// hector_amd.h defines every operation and its order; contraction is off as in the score kernel).
// One lane per member, nothing exchanged between lanes; blockIdx.y picks a GROUP of up to
// HXM_GROUP specifications whose state lives in registers.  The host (EnsembleCore::metric_block)
// hands every group two ascending row lists -- the union of its reference periods, the union of
// its windows -- so that the specifications of a group read a row they share once, and the
// reference means are complete before the windows are consumed.  The score kernel has one dependent
// load of a lane in flight; here a lane takes HXM_BATCH rows into registers, all loads in flight,
// and the next batch is issued before the current one is consumed in the defined order.  The group
// record and the row lists are wave-uniform reads of constant memory (scalar loads).
// HXM_GROUP, HXM_BATCH, HXM_PAD, HxMetSpec and HxMetGroup: hx_post_abi.h.
// ===========================================================================

// (the row numbers are read again from the list when the batch is consumed -- scalar loads that hit
//  the scalar cache -- instead of being held in 2 x HXM_BATCH scalar registers across the loop)
__device__ __forceinline__ void hxm_load(const double *col, int npad, const int *r, double (&x)[HXM_BATCH]) {
#pragma unroll
  for (int e = 0; e < HXM_BATCH; ++e)
    x[e] = col[(size_t)(r[e] & (HXM_PAD - 1)) * (size_t)npad];
}

#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__device__ __forceinline__ void hxm_base_batch(const HxMetGroup &g, const int *__restrict__ iy,
                                               const double (&x)[HXM_BATCH], double (&bs)[HXM_GROUP],
                                               unsigned (&bbad)[HXM_GROUP]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
  for (int k = 0; k < HXM_GROUP; ++k) {
    if (k >= g.nbase) continue;
    const int b0 = g.b0[k], b1 = g.b1[k];
#pragma unroll
    for (int e = 0; e < HXM_BATCH; ++e)
      if (iy[e] >= b0 && iy[e] <= b1) {
        bs[k] = bs[k] + x[e];
        bbad[k] |= x[e] != x[e] ? 1u : 0u;
      }
  }
}

// one specification over one batch of rows, in row order.  sb = +0.0 without a reference period
// (x - 0.0 is x, bit for bit).  Four code paths: MEAN; MIN / MAX and their years (MAX as the MIN of
// the negated values: negation is exact and strict > becomes strict <); the two _GE operations
// (count in acc, first year in aux); SLOPE.
#define HXM_PATH_MEAN 0
#define HXM_PATH_EXT 1
#define HXM_PATH_GE 2
#define HXM_PATH_SLOPE 3
template <int PATH>
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__device__ __forceinline__ void hxm_spec_batch(int iy0, int iy1, bool negate, double thr, double mid,
                                               const int *__restrict__ iy, const double (&x)[HXM_BATCH],
                                               double sb, int year_start, double &acc, double &aux,
                                               double &den, unsigned &bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
  for (int e = 0; e < HXM_BATCH; ++e) {
    if (iy[e] < iy0 || iy[e] > iy1) continue;   // wave-uniform
    const double xv = x[e];
    bad |= xv != xv ? 1u : 0u;   // (a lane flag in a vector register, not a mask in scalar ones)
    const double a = xv - sb;
    const double yd = (double)(year_start + iy[e]);
    if (PATH == HXM_PATH_MEAN) {
      acc = acc + a;
    } else if (PATH == HXM_PATH_EXT) {
      const double c = negate ? -a : a;
      if (iy[e] == iy0 || c < acc) { acc = c; aux = yd; }
    } else if (PATH == HXM_PATH_GE) {
      const bool ge = a >= thr;
      acc = acc + (ge ? 1.0 : 0.0);
      if (ge && aux != aux) aux = yd;
    } else {
      const double t = yd - mid;
      const double p = t * a;
      acc = acc + p;
      const double tt = t * t;
      den = den + tt;
    }
  }
}

__device__ __forceinline__ int hxm_path(int op) {
  return op == HX_MET_MEAN ? HXM_PATH_MEAN
         : op == HX_MET_SLOPE ? HXM_PATH_SLOPE
         : (op == HX_MET_FIRST_GE || op == HX_MET_COUNT_GE) ? HXM_PATH_GE : HXM_PATH_EXT;
}

// out[(group * HXM_GROUP + j)][npad] in lane order; lanes >= n are not written
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_metric_kernel(const double *__restrict__ var, int n, int npad,
                                                        const HxMetGroup *__restrict__ groups,
                                                        const int *__restrict__ rows, int year_start,
                                                        double *__restrict__ out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= n) return;
  const HxMetGroup &g = groups[blockIdx.y];
  const double *col = var + lane;
  const int nspec = g.nspec, nbase = g.nbase;
  double xa[HXM_BATCH], xb[HXM_BATCH];
  // the reference means of the group
  double bs[HXM_GROUP];
  unsigned bbad[HXM_GROUP];
#pragma unroll
  for (int k = 0; k < HXM_GROUP; ++k) { bs[k] = 0.0; bbad[k] = 0u; }
  if (g.nbrow > 0) {
    const int *r = rows + g.brow0;
    const int nrow = g.nbrow;
    hxm_load(col, npad, r, xa);
    for (int i = 0; i < nrow; i += HXM_BATCH) {
      const bool more = i + HXM_BATCH < nrow;
      if (more) hxm_load(col, npad, r + i + HXM_BATCH, xb);   // in flight while this batch is consumed
      hxm_base_batch(g, r + i, xa, bs, bbad);
      if (more) {
#pragma unroll
        for (int e = 0; e < HXM_BATCH; ++e) xa[e] = xb[e];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < HXM_GROUP; ++k)
    if (k < nbase) bs[k] = bs[k] / (double)(g.b1[k] - g.b0[k] + 1);
  int op[HXM_GROUP], iy0[HXM_GROUP], iy1[HXM_GROUP];
  double thr[HXM_GROUP], mid[HXM_GROUP];
  double acc[HXM_GROUP], aux[HXM_GROUP], den[HXM_GROUP], sb[HXM_GROUP];
  unsigned bad[HXM_GROUP];
#pragma unroll
  for (int j = 0; j < HXM_GROUP; ++j) {
    acc[j] = 0.0; den[j] = 0.0; aux[j] = __builtin_nan(""); sb[j] = 0.0; bad[j] = 0u;
    op[j] = g.s[j].op; iy0[j] = g.s[j].iy0; iy1[j] = g.s[j].iy1; thr[j] = g.s[j].thr; mid[j] = g.s[j].mid;
    const int b = g.s[j].base;
#pragma unroll
    for (int k = 0; k < HXM_GROUP; ++k)
      if (b == k) { sb[j] = bs[k]; bad[j] = bbad[k]; }
  }
  {
    const int *r = rows + g.wrow0;
    const int nrow = g.nwrow;
    hxm_load(col, npad, r, xa);
    for (int i = 0; i < nrow; i += HXM_BATCH) {
      const bool more = i + HXM_BATCH < nrow;
      if (more) hxm_load(col, npad, r + i + HXM_BATCH, xb);
#pragma unroll
      for (int j = 0; j < HXM_GROUP; ++j) {
        if (j >= nspec) continue;
        const bool neg = op[j] == HX_MET_MAX || op[j] == HX_MET_YEAR_OF_MAX;
        switch (hxm_path(op[j])) {   // wave-uniform
          case HXM_PATH_MEAN:
            hxm_spec_batch<HXM_PATH_MEAN>(iy0[j], iy1[j], neg, thr[j], mid[j], r + i, xa, sb[j], year_start,
                                          acc[j], aux[j], den[j], bad[j]); break;
          case HXM_PATH_EXT:
            hxm_spec_batch<HXM_PATH_EXT>(iy0[j], iy1[j], neg, thr[j], mid[j], r + i, xa, sb[j], year_start,
                                         acc[j], aux[j], den[j], bad[j]); break;
          case HXM_PATH_GE:
            hxm_spec_batch<HXM_PATH_GE>(iy0[j], iy1[j], neg, thr[j], mid[j], r + i, xa, sb[j], year_start,
                                        acc[j], aux[j], den[j], bad[j]); break;
          default:
            hxm_spec_batch<HXM_PATH_SLOPE>(iy0[j], iy1[j], neg, thr[j], mid[j], r + i, xa, sb[j], year_start,
                                           acc[j], aux[j], den[j], bad[j]); break;
        }
      }
      if (more) {
#pragma unroll
        for (int e = 0; e < HXM_BATCH; ++e) xa[e] = xb[e];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < HXM_GROUP; ++j) {
    if (j >= nspec) continue;
    const int o = op[j];
    double v = acc[j];                                   // MIN, COUNT_GE
    if (o == HX_MET_MAX) v = -acc[j];
    if (o == HX_MET_YEAR_OF_MIN || o == HX_MET_YEAR_OF_MAX || o == HX_MET_FIRST_GE) v = aux[j];
    if (o == HX_MET_MEAN || o == HX_MET_SLOPE) {
      const double d = o == HX_MET_MEAN ? (double)(iy1[j] - iy0[j] + 1) : den[j];
      v = acc[j] / d;
    }
    if (bad[j]) v = __builtin_nan("");
    out[((size_t)blockIdx.y * HXM_GROUP + (size_t)j) * (size_t)npad + (size_t)lane] = v;
  }
}

hipError_t hx_launch_metric(const double *var, int n, int npad, const void *groups, int ngroups,
                            const int *rows, int year_start, double *out, hipStream_t st) {
  hipLaunchKernelGGL(hx_metric_kernel, dim3((n + 255) / 256, ngroups), dim3(256), 0, st, var, n, npad,
                     (const HxMetGroup *)groups, rows, year_start, out);
  return hipGetLastError();
}

// ===========================================================================
// Series: kept [ns][npad] blocks in lane order that small lane-local kernels fill from a source
// block (hx_series_define in hector_amd.h defines every operation and its order; contraction is
// off as in the score kernel).  One lane per member, rows read coalesced, nothing exchanged between
// lanes.  Every kernel writes ALL ns rows of z: NaN where the operation has no value.
//   hx_series_ew_kernel     the elementwise operations, a pure stream: a lane takes HXS_BATCH rows of
//                           each operand into registers, all loads in flight, then computes and stores
//   hx_series_base_kernel   the lane's own mean over a reference period (ANOMALY's first step)
//   hx_series_cumsum_kernel walks the years of a lane; the next batch of rows is in flight while the
//                           running sum consumes the current one
//   hx_series_runmean_kernel one (lane, year) per thread: a FRESH ascending sum of the window, whose
//                           rows neighbouring years re-read from L2
//   hx_series_permute_kernel a block into another lane order
// ===========================================================================
#define HXS_BATCH 16   // (the internal ops HXS_ANOM_APPLY and HXS_COMBINE: hx_post_abi.h)

template <int OP>
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__device__ __forceinline__ double hxs_apply(double a, double b, double c0, double c1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (OP == HX_SER_ADD) return a + b;
  if (OP == HX_SER_SUB || OP == HXS_ANOM_APPLY) return a - b;
  if (OP == HX_SER_MUL) return a * b;
  if (OP == HX_SER_DIV) return a / b;
  if (OP == HXS_COMBINE) { const double p = c0 * a; const double q = c1 * b; return p + q; }
  return a;   // HX_SER_COPY
}

// rows y_lo..y_hi are computed, every other row of 0..ns-1 is NaN.  b != nullptr: a block (DELTA
// passes a itself k rows earlier: rows below y_lo = k are never loaded); else bvec[ns], one value a
// year for every lane (a wave-uniform read); HXS_ANOM_APPLY: base[lane].  grid (lanes / 256, years /
// HXS_BATCH)
template <int OP>
__global__ __launch_bounds__(256) void hx_series_ew_kernel(const double *__restrict__ a,
                                                           const double *__restrict__ b,
                                                           const double *__restrict__ bvec,
                                                           const double *__restrict__ base, int npad, int ns,
                                                           int y_lo, int y_hi, double c0, double c1,
                                                           double *__restrict__ z) {
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const int y0 = (int)blockIdx.y * HXS_BATCH;
  constexpr bool unary = OP == HX_SER_COPY || OP == HXS_ANOM_APPLY;
  double xa[HXS_BATCH], xb[HXS_BATCH];
#pragma unroll
  for (int e = 0; e < HXS_BATCH; ++e) {
    const int y = y0 + e;
    const bool on = y >= y_lo && y <= y_hi;   // wave-uniform
    xa[e] = 0.0; xb[e] = 0.0;
    if (on) {
      xa[e] = a[(size_t)y * (size_t)npad + (size_t)lane];
      if (!unary) xb[e] = b ? b[(size_t)y * (size_t)npad + (size_t)lane] : bvec[y];
    }
  }
  const double bl = OP == HXS_ANOM_APPLY ? base[lane] : 0.0;
#pragma unroll
  for (int e = 0; e < HXS_BATCH; ++e) {
    const int y = y0 + e;
    if (y >= ns) continue;
    const bool on = y >= y_lo && y <= y_hi;
    const double r = hxs_apply<OP>(xa[e], OP == HXS_ANOM_APPLY ? bl : xb[e], c0, c1);
    z[(size_t)y * (size_t)npad + (size_t)lane] = on ? r : __builtin_nan("");
  }
}

// base[lane] = (sum of a over the rows r0..r1 ascending, starting from 0.0) / count
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_series_base_kernel(const double *__restrict__ a, int npad, int r0,
                                                             int r1, double *__restrict__ base) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const double *col = a + lane;
  double s = 0.0;
  for (int k = r0; k <= r1; k += HXS_BATCH) {
    double x[HXS_BATCH];
#pragma unroll
    for (int e = 0; e < HXS_BATCH; ++e) x[e] = k + e <= r1 ? col[(size_t)(k + e) * (size_t)npad] : 0.0;
#pragma unroll
    for (int e = 0; e < HXS_BATCH; ++e) if (k + e <= r1) s = s + x[e];
  }
  base[lane] = s / (double)(r1 - r0 + 1);
}

// NaN before row y0; z_y0 = a_y0, z_y = z_(y-1) + a_y up to row y_hi; NaN behind it
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_series_cumsum_kernel(const double *__restrict__ a, int npad, int ns,
                                                               int y0, int y_hi, double *__restrict__ z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const double *col = a + lane;
  double *out = z + lane;
  const double nan = __builtin_nan("");
  for (int y = 0; y < y0; ++y) out[(size_t)y * (size_t)npad] = nan;
  double xa[HXS_BATCH], xb[HXS_BATCH];
  auto load = [&](int k, double (&x)[HXS_BATCH]) {
#pragma unroll
    for (int e = 0; e < HXS_BATCH; ++e) x[e] = k + e <= y_hi ? col[(size_t)(k + e) * (size_t)npad] : 0.0;
  };
  double s = 0.0;
  load(y0, xa);
  for (int k = y0; k <= y_hi; k += HXS_BATCH) {
    const bool more = k + HXS_BATCH <= y_hi;
    if (more) load(k + HXS_BATCH, xb);   // in flight while this batch is consumed
#pragma unroll
    for (int e = 0; e < HXS_BATCH; ++e) {
      if (k + e > y_hi) continue;
      s = k + e == y0 ? xa[e] : s + xa[e];
      out[(size_t)(k + e) * (size_t)npad] = s;
    }
    if (more) {
#pragma unroll
      for (int e = 0; e < HXS_BATCH; ++e) xa[e] = xb[e];
    }
  }
  for (int y = y_hi + 1; y < ns; ++y) out[(size_t)y * (size_t)npad] = nan;
}

// z_y = (fresh ascending sum of a over the rows y - back .. y - back + w - 1, from 0.0) / w; NaN
// where the window leaves 0..y_hi.  grid (lanes / 256, ns)
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_series_runmean_kernel(const double *__restrict__ a, int npad, int w,
                                                                int back, int y_hi, double *__restrict__ z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const int y = (int)blockIdx.y;
  const int wl = y - back, wh = wl + w - 1;   // (w <= ns is checked by the host: no overflow)
  double r = __builtin_nan("");
  if (wl >= 0 && wh <= y_hi) {
    const double *col = a + lane;
    double s = 0.0;
    for (int k = wl; k <= wh; k += HXS_BATCH) {
      double x[HXS_BATCH];
#pragma unroll
      for (int e = 0; e < HXS_BATCH; ++e) x[e] = k + e <= wh ? col[(size_t)(k + e) * (size_t)npad] : 0.0;
#pragma unroll
      for (int e = 0; e < HXS_BATCH; ++e) if (k + e <= wh) s = s + x[e];
    }
    r = s / (double)w;
  }
  z[(size_t)y * (size_t)npad + (size_t)lane] = r;
}

// dst[y][l] = src[y][src_lane[l]]: a block into another lane order.  grid (lanes / 256, ns)
__global__ __launch_bounds__(256) void hx_series_permute_kernel(const double *__restrict__ src,
                                                                const int *__restrict__ src_lane, int npad,
                                                                double *__restrict__ dst) {
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const size_t row = (size_t)blockIdx.y * (size_t)npad;
  dst[row + (size_t)lane] = src[row + (size_t)src_lane[lane]];
}

hipError_t hx_launch_series_ew(int op, const double *a, const double *b, const double *bvec, const double *base,
                               int npad, int ns, int y_lo, int y_hi, double c0, double c1, double *z,
                               hipStream_t st) {
  const dim3 grid((npad + 255) / 256, (ns + HXS_BATCH - 1) / HXS_BATCH), block(256);
#define HXS_EW(OP) \
  hipLaunchKernelGGL(hx_series_ew_kernel<OP>, grid, block, 0, st, a, b, bvec, base, npad, ns, y_lo, y_hi, c0, c1, z)
  switch (op) {
    case HX_SER_COPY: HXS_EW(HX_SER_COPY); break;
    case HX_SER_ADD: HXS_EW(HX_SER_ADD); break;
    case HX_SER_SUB: HXS_EW(HX_SER_SUB); break;
    case HX_SER_MUL: HXS_EW(HX_SER_MUL); break;
    case HX_SER_DIV: HXS_EW(HX_SER_DIV); break;
    case HXS_ANOM_APPLY: HXS_EW(HXS_ANOM_APPLY); break;
    case HXS_COMBINE: HXS_EW(HXS_COMBINE); break;
    default: return hipErrorInvalidValue;
  }
#undef HXS_EW
  return hipGetLastError();
}
hipError_t hx_launch_series_base(const double *a, int npad, int r0, int r1, double *base, hipStream_t st) {
  hipLaunchKernelGGL(hx_series_base_kernel, dim3((npad + 255) / 256), dim3(256), 0, st, a, npad, r0, r1, base);
  return hipGetLastError();
}
hipError_t hx_launch_series_cumsum(const double *a, int npad, int ns, int y0, int y_hi, double *z,
                                   hipStream_t st) {
  hipLaunchKernelGGL(hx_series_cumsum_kernel, dim3((npad + 255) / 256), dim3(256), 0, st, a, npad, ns, y0,
                     y_hi, z);
  return hipGetLastError();
}
hipError_t hx_launch_series_runmean(const double *a, int npad, int ns, int w, int back, int y_hi, double *z,
                                    hipStream_t st) {
  hipLaunchKernelGGL(hx_series_runmean_kernel, dim3((npad + 255) / 256, ns), dim3(256), 0, st, a, npad, w,
                     back, y_hi, z);
  return hipGetLastError();
}
hipError_t hx_launch_series_permute(const double *src, const int *src_lane, int npad, int ns, double *dst,
                                    hipStream_t st) {
  hipLaunchKernelGGL(hx_series_permute_kernel, dim3((npad + 255) / 256, ns), dim3(256), 0, st, src, src_lane,
                     npad, dst);
  return hipGetLastError();
}

#include "hx_dev_expr.h"   // hx_series_eval: a series from a whole expression in one launch

// ===========================================================================
// Per-member input series as a mix of shared year-vectors (hx_setvar_dated_mix in hector_amd.h
// defines the value and its order; contraction is off as in the score kernel): the [row][npad]
// table the run kernels read behind an ms_mask bit, built on the device.
//   fill: table[r][lane] = row[r] for every row -- the shared series under a mix that has no dense
//         table beneath it.  grid (lanes / 256, ns)
//   mix:  table[rows[i]][lane] = sum over k, ascending, of coeff[k][member(lane)] * basis[k][i], each
//         product rounded before it is added.  The lane takes its coefficients once through
//         member_of_lane (a padding lane: the last member's, as the dense upload does) and writes
//         its element of HXMIX_TILE covered rows; rows[] and basis[] are indexed by blockIdx.y and
//         the loop counter alone, so they stay in scalar registers.  grid (lanes / 256,
//         ceil(nrows / HXMIX_TILE)): 65 536 lanes x 71 rows are 2304 blocks.  Lane-local: nothing
//         is exchanged, the host-emulation build runs it as it stands.
// ===========================================================================
#define HXMIX_TILE 8
__global__ __launch_bounds__(256) void hx_mseries_fill_kernel(const double *__restrict__ row, int npad,
                                                              double *__restrict__ table) {
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  table[(size_t)blockIdx.y * (size_t)npad + (size_t)lane] = row[blockIdx.y];
}

#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_mseries_mix_kernel(const double *__restrict__ coeff,
                                                             const int *__restrict__ member_of_lane, int n,
                                                             int npad, const int *__restrict__ rows,
                                                             const double *__restrict__ basis, int nrows,
                                                             int nbasis, double *__restrict__ table) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const int m = min(member_of_lane[lane], n - 1);
  double c[HX_MIX_MAX_BASIS];
#pragma unroll
  for (int k = 0; k < HX_MIX_MAX_BASIS; ++k) c[k] = k < nbasis ? coeff[(size_t)k * (size_t)n + (size_t)m] : 0.0;
  const int i0 = (int)blockIdx.y * HXMIX_TILE, i1 = min(i0 + HXMIX_TILE, nrows);
  for (int i = i0; i < i1; ++i) {
    double s = c[0] * basis[i];
#pragma unroll
    for (int k = 1; k < HX_MIX_MAX_BASIS; ++k)
      if (k < nbasis) {
        const double p = c[k] * basis[(size_t)k * (size_t)nrows + (size_t)i];
        s = s + p;
      }
    table[(size_t)rows[i] * (size_t)npad + (size_t)lane] = s;
  }
}

hipError_t hx_launch_mseries_fill(const double *row, int ns, int npad, double *table, hipStream_t st) {
  hipLaunchKernelGGL(hx_mseries_fill_kernel, dim3((npad + 255) / 256, ns), dim3(256), 0, st, row, npad, table);
  return hipGetLastError();
}
hipError_t hx_launch_mseries_mix(const double *coeff, const int *member_of_lane, int n, int npad, const int *rows,
                                 const double *basis, int nrows, int nbasis, double *table, hipStream_t st) {
  if (nrows < 1 || nbasis < 1 || nbasis > HX_MIX_MAX_BASIS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hx_mseries_mix_kernel, dim3((npad + 255) / 256, (nrows + HXMIX_TILE - 1) / HXMIX_TILE),
                     dim3(256), 0, st, coeff, member_of_lane, n, npad, rows, basis, nrows, nbasis, table);
  return hipGetLastError();
}

// ===========================================================================
// The gas pre-pass from RECIPES: hx_gas_kernel's two rows (N2O[t]; halocarbon + albedo + misc
// forcing) for a core in which a member's N2O_emissions, RF_albedo or <gas>_emissions is a mix
// (hx_setvar_dated_mix).  No [ns][npad] table of emissions exists: the lane takes the coefficients of
// ONE input at a time through member_of_lane (a padding lane: the last member's), evaluates the
// definition in every covered year -- products rounded before they are added, ascending k, as
// hx_mseries_mix_kernel does -- and takes the shared value elsewhere.  The value chain is the host's
// (EnsembleCore::build_shared), operation for operation, contraction off.
//   par [3 + 3 nh][npad], ser [4 + 2 nh][ns], h0 [nh]: as hx_gas_kernel, gases in the order their
//       forcings are summed
//   nat [ns]: N2O_natural_emissions;  molar [nh]: molar masses
//   rec [2 + nh][2]: input j's {nbasis (0 = shared), index of its block}: j = 0 N2O_emissions,
//       1 RF_albedo, 2 + h the emissions of gas h.  Block b: coeff + coff[b] is [nbasis][n] in member
//       order, basis + b * HX_MIX_MAX_BASIS * ns is [nbasis][ns] dense in years, cover + b * ns is
//       non-zero in the years the mix lists.  basis, cover, ser, nat and rec are indexed by the loop
//       counters alone: scalar loads.
// Gases OUTSIDE, years inside: a lane holds one input's (at most 8) coefficients and one recurrence;
// the forcing row is accumulated in memory in the host's order -- 0.0 + gas 0 + gas 1 ..., then
// (that + albedo) + misc -- so (nh + 1) read-modify-writes of a coalesced row per year.  Lane-local:
// the host-emulation build runs it as it stands.
// ===========================================================================
// the definition's value in year iy from the coefficients c[] and the basis block b (K vectors)
#define HX_GASMIX_VALUE(dst, iy)                                              \
  do {                                                                        \
    double s_ = c[0] * b[iy];                                                 \
    _Pragma("unroll") for (int k_ = 1; k_ < HX_MIX_MAX_BASIS; ++k_)           \
      if (k_ < K) {                                                           \
        const double p_ = c[k_] * b[(size_t)k_ * (size_t)ns + (size_t)(iy)];  \
        s_ = s_ + p_;                                                         \
      }                                                                       \
    dst = s_;                                                                 \
  } while (0)

#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(64) void hx_gas_mix_kernel(const double *__restrict__ par, const double *__restrict__ ser,
                                                        const double *__restrict__ h0, const double *__restrict__ nat,
                                                        const double *__restrict__ molar, const int *__restrict__ rec,
                                                        const double *__restrict__ coeff, const long long *__restrict__ coff,
                                                        const double *__restrict__ basis, const int *__restrict__ cover,
                                                        const int *__restrict__ member_of_lane, int n, int nh, int ns,
                                                        int npad, double *__restrict__ n2o_out,
                                                        double *__restrict__ rf_other_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const size_t np = (size_t)npad, mem = (size_t)lane;
  const size_t m = (size_t)min(member_of_lane[lane], n - 1);
  double c[HX_MIX_MAX_BASIS];
  auto take = [&](int j, const double *&b, const int *&cov) {   // input j's recipe; returns nbasis
    const int K = rec[2 * j], blk = rec[2 * j + 1];
#pragma unroll
    for (int k = 0; k < HX_MIX_MAX_BASIS; ++k) c[k] = k < K ? coeff[coff[blk] + (long long)((size_t)k * (size_t)n + m)] : 0.0;
    b = basis + (size_t)blk * HX_MIX_MAX_BASIS * (size_t)ns;
    cov = cover + (size_t)blk * (size_t)ns;
    return K;
  };
  const double *b = nullptr;
  const int *cov = nullptr;
  {  // N2OComponent::run (src/n2o_component.cpp:152-191)
    const double N0 = par[mem], TN2O0 = par[np + mem], UC = par[2 * np + mem];
    const double *em = ser, *ncon = ser + ns;
    const int K = rec[0] ? take(0, b, cov) : 0;
    const double N0f = isnan(ncon[0]) ? N0 : ncon[0];
    double n2o = N0f;
    n2o_out[mem] = n2o;
    for (int iy = 1; iy < ns; ++iy) {
      const double tau_n = TN2O0 * pow(n2o / N0f, -0.05);
      double e = em[iy];
      if (K && cov[iy]) {
        double v;
        HX_GASMIX_VALUE(v, iy);
        e = v + nat[iy];
      }
      n2o = n2o + (e / UC - n2o / tau_n);
      if (!isnan(ncon[iy])) n2o = ncon[iy];
      n2o_out[(size_t)iy * np + mem] = n2o;
    }
  }
  // HalocarbonComponent::run (src/halocarbon_component.cpp:181-229), one gas after the other
  for (int h = 0; h < nh; ++h) {
    const double tau = par[(size_t)(3 + 3 * h) * np + mem], rho = par[(size_t)(4 + 3 * h) * np + mem],
                 delta = par[(size_t)(5 + 3 * h) * np + mem];
    const double expfac = exp(-(1 / tau));
    const double *dser = ser + (size_t)(4 + 2 * h) * ns, *hcon = ser + (size_t)(5 + 2 * h) * ns;
    const double mm = molar[h];
    const int K = rec[2 * (2 + h)] ? take(2 + h, b, cov) : 0;
    double conc = h0[h];
    for (int iy = 1; iy < ns; ++iy) {
      double dconc = dser[iy];
      if (K && cov[iy]) {
        double v;
        HX_GASMIX_VALUE(v, iy);
        const double emissMol = v / mm * 1.0;
        dconc = emissMol / (0.1 * 1.8);
      }
      conc = conc * expfac + dconc * tau * (1.0 - expfac);
      if (!isnan(hcon[iy])) conc = hcon[iy];
      const double rf_un = rho * conc;
      const size_t o = (size_t)iy * np + mem;
      const double before = h == 0 ? 0.0 : rf_other_out[o];
      rf_other_out[o] = before + (rf_un + delta * rf_un);
    }
  }
  {  // + RF_albedo + RF_misc (ForcingComponent::run, src/forcing_component.cpp:400-487)
    const double *alb = ser + 2 * (size_t)ns, *misc = ser + 3 * (size_t)ns;
    const int K = rec[2] ? take(1, b, cov) : 0;
    for (int iy = 0; iy < ns; ++iy) {
      const size_t o = (size_t)iy * np + mem;
      double a = alb[iy];
      if (K && cov[iy]) HX_GASMIX_VALUE(a, iy);
      const double rf_h = (nh == 0 || iy == 0) ? 0.0 : rf_other_out[o];
      rf_other_out[o] = (rf_h + a) + misc[iy];
    }
  }
}

hipError_t hx_launch_gas_mix(const double *par, const double *ser, const double *h0, const double *nat,
                             const double *molar, const int *rec, const double *coeff, const long long *coff,
                             const double *basis, const int *cover, const int *member_of_lane, int n, int nh,
                             int ns, int npad, double *n2o_out, double *rf_other_out, hipStream_t st) {
  if (n < 1 || nh < 0 || ns < 1 || npad < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hx_gas_mix_kernel, dim3((npad + 63) / 64), dim3(64), 0, st, par, ser, h0, nat, molar, rec,
                     coeff, coff, basis, cover, member_of_lane, n, nh, ns, npad, n2o_out, rf_other_out);
  return hipGetLastError();
}

// ===========================================================================
// The aerosol and ozone / OH precursor terms from RECIPES: the per-member counterparts of seven
// columns of the per-year table (HXM_OH_B .. HXM_RF_AERO in hx_layout.h) for a core in which a
// member's SO2 / BC / OC / NH3 or NOX / CO / NMVOC emissions are a mix (hx_setvar_dated_mix).  Like
// hx_gas_mix_kernel there is no table of emissions: the lane takes its coefficients through
// member_of_lane (a padding lane: the last member's), evaluates the definition in every covered
// year -- products rounded before they are added, ascending k -- and takes the scenario's value
// elsewhere.  The rows are written with the expressions of EnsembleCore::build_shared, operation for
// operation, contraction off, and they are the TERMS, not their sums: the year loop adds them.
// Unlike the gas pre-pass nothing here is a recurrence -- a year's terms depend on that year's
// emissions, and the OH terms on the member's own value at startDate besides -- so a block takes
// 64 lanes x HXSLCF_YEARS years: grid (npad / 64, ceil(ns / HXSLCF_YEARS)).
//   ser [12][ns]: the scenario's SO2, BC, OC, NH3; NOX, CO, NMVOC of the OH section; the same of the
//       ozone section; then the argument of the aerosol-cloud logarithm for the scenario's own
//       emissions and the host's term for it (the shared column's std::log)
//   kon [8]: rho_bc, rho_oc, rho_so2, rho_nh3, CNOX, CCO, CNMVOC, and non-zero if one of the four aerosol
//       components is disabled (the row is zero then, as the shared column is)
//   rec [7][2]: input j's {nbasis (0 = shared), block}: j = 0 SO2, 1 BC, 2 OC, 3 NH3, 4 NOX, 5 CO,
//       6 NMVOC; coeff, coff, basis, cover: as hx_gas_mix_kernel
//   rows.r[k]: row HXM_OH_B + k, [ns][npad]; r[0..5] null: no precursor group; r[6] null: no aerosol row
//   rho.r[j]: rho_bc, rho_oc, rho_so2, rho_nh3 of every member, [n] in member order (read through
//       member_of_lane as the coefficients are), or null: the scalar in kon (hx_enable_member_forcing)
// The logarithm is the device library's.  Where a member's argument IS the scenario's, bit for bit,
// the lane takes the host's term: a member that carries the scenario's own aerosol emissions then
// has the bits of a core without the mix (the two logarithms differ in the last place now and then).
// Lane-local: the host-emulation build runs it as it stands.
// ===========================================================================
#define HXSLCF_YEARS 64
struct HxSlcfRows { double *r[7]; };
struct HxSlcfRho { const double *r[4]; };

#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(64) void hx_slcf_mix_kernel(const double *__restrict__ ser, const double *__restrict__ kon,
                                                         const int *__restrict__ rec, const double *__restrict__ coeff,
                                                         const long long *__restrict__ coff,
                                                         const double *__restrict__ basis, const int *__restrict__ cover,
                                                         const int *__restrict__ member_of_lane, int n, int ns, int npad,
                                                         HxSlcfRows rows, HxSlcfRho rho) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const size_t np = (size_t)npad, mem = (size_t)lane;
  const size_t m = (size_t)min(member_of_lane[lane], n - 1);
  const int iy0 = (int)blockIdx.y * HXSLCF_YEARS, iy1 = min(iy0 + HXSLCF_YEARS, ns);
  if (rows.r[0]) {  // OHComponent::run (src/oh_component.cpp:157-170), OzoneComponent::run (src/o3_component.cpp:136-139)
    const double o3f[3] = {0.125, 0.0011, 0.0033};
    for (int p = 0; p < 3; ++p) {
      const int K = rec[2 * (4 + p)], blk = rec[2 * (4 + p) + 1];
      double c[HX_MIX_MAX_BASIS];
#pragma unroll
      for (int k = 0; k < HX_MIX_MAX_BASIS; ++k) c[k] = k < K ? coeff[coff[blk] + (long long)((size_t)k * (size_t)n + m)] : 0.0;
      const double *b = basis + (size_t)blk * HX_MIX_MAX_BASIS * (size_t)ns;
      const int *cov = cover + (size_t)blk * (size_t)ns;
      const double *soh = ser + (size_t)(4 + p) * ns, *so3 = ser + (size_t)(7 + p) * ns;
      const double C = kon[4 + p], F = o3f[p];
      double x0 = soh[0];   // the member's own emissions of startDate when the mix covers it
      if (K && cov[0]) HX_GASMIX_VALUE(x0, 0);
      double *oh = rows.r[p], *o3 = rows.r[3 + p];
      for (int iy = iy0; iy < iy1; ++iy) {
        double xo = soh[iy], xz = so3[iy];
        if (K && cov[iy]) {
          double v;
          HX_GASMIX_VALUE(v, iy);
          xo = xz = v;
        }
        const size_t o = (size_t)iy * np + mem;
        oh[o] = C * ((1.0 * xo) - x0);
        o3[o] = F * xz;
      }
    }
  }
  if (rows.r[6]) {  // ForcingComponent::run (src/forcing_component.cpp:430-470) for aero_scalar = 1
    const double aci_beta = 2.279759, s_BCOC = 111.05064063;
    const double s_SO2 = (260.34644166 * 1000) * (32.065 / 64.066);
    const double rho_bc = rho.r[0] ? rho.r[0][m] : kon[0], rho_oc = rho.r[1] ? rho.r[1][m] : kon[1];
    const double rho_so2 = rho.r[2] ? rho.r[2][m] : kon[2], rho_nh3 = rho.r[3] ? rho.r[3][m] : kon[3];
    const double *arg_sh = ser + (size_t)10 * ns, *aci_sh = ser + (size_t)11 * ns;
    double ca[4][HX_MIX_MAX_BASIS];
    int Ka[4];
    const double *ba[4];
    const int *cva[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Ka[j] = rec[2 * j];
      const int blk = rec[2 * j + 1];
#pragma unroll
      for (int k = 0; k < HX_MIX_MAX_BASIS; ++k)
        ca[j][k] = k < Ka[j] ? coeff[coff[blk] + (long long)((size_t)k * (size_t)n + m)] : 0.0;
      ba[j] = basis + (size_t)blk * HX_MIX_MAX_BASIS * (size_t)ns;
      cva[j] = cover + (size_t)blk * (size_t)ns;
    }
    double *out = rows.r[6];
    for (int iy = iy0; iy < iy1; ++iy) {
      double e[4];   // SO2, BC, OC, NH3 of the year
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = ser[(size_t)j * ns + iy];
        if (Ka[j] && cva[j][iy]) {
          double s = ca[j][0] * ba[j][iy];
#pragma unroll
          for (int k = 1; k < HX_MIX_MAX_BASIS; ++k)
            if (k < Ka[j]) {
              const double p = ca[j][k] * ba[j][(size_t)k * (size_t)ns + (size_t)iy];
              s = s + p;
            }
          e[j] = s;
        }
      }
      const double so2 = e[0], bc = e[1], oc = e[2], nh3 = e[3];
      const double arg = 1 + (so2 / s_SO2) + ((bc + oc) / s_BCOC);
      const double aci = arg == arg_sh[iy] ? aci_sh[iy] : -1 * aci_beta * log(arg);
      const double rf = (((rho_bc * bc + rho_oc * oc) + rho_so2 * so2) + rho_nh3 * nh3) + aci;
      out[(size_t)iy * np + mem] = kon[7] != 0.0 ? 0.0 : rf;
    }
  }
}

hipError_t hx_launch_slcf_mix(const double *ser, const double *kon, const int *rec, const double *coeff,
                              const long long *coff, const double *basis, const int *cover,
                              const int *member_of_lane, int n, int ns, int npad, double *const *rows7,
                              const double *const *rho4, hipStream_t st) {
  if (n < 1 || ns < 1 || npad < 1) return hipErrorInvalidValue;
  HxSlcfRows rows;
  for (int k = 0; k < 7; ++k) rows.r[k] = rows7[k];
  HxSlcfRho rho;
  for (int j = 0; j < 4; ++j) rho.r[j] = rho4 ? rho4[j] : nullptr;
  hipLaunchKernelGGL(hx_slcf_mix_kernel, dim3((npad + 63) / 64, (ns + HXSLCF_YEARS - 1) / HXSLCF_YEARS), dim3(64), 0,
                     st, ser, kon, rec, coeff, coff, basis, cover, member_of_lane, n, ns, npad, rows, rho);
  return hipGetLastError();
}
#undef HX_GASMIX_VALUE

// ===========================================================================
// Pair metrics: one double per member from a window of TWO series of that member, a (reported /
// dependent) and b (condition / independent) -- hx_member_pair_metrics in hector_amd.h defines every
// operation and its order; contraction is off as in the score kernel.  One lane per member, nothing
// exchanged between lanes; blockIdx.y picks ONE specification, whose record is a wave-uniform read
// (scalar loads).  No grouping: a second specification re-reads its rows from L2.
// Phases: the reference rows of a, the reference rows of b, the window (pass 1), and the window again
// (pass 2) for SLOPE / INTERCEPT / R2 only; END_RATIO reads its two end rows instead of the window.
// Every phase walks CONSECUTIVE rows, so there are no row lists: a lane takes HXP_BATCH rows of each
// operand into registers, all loads in flight, and the next batch is issued before the current one is
// consumed in the defined order (hxm_load's pattern; rows past the phase's last one are loaded from
// that last row and never consumed).  BVEC: b is the caller's per-year vector, bvec[iy - bvec_iy0],
// the same for every lane -- wave-uniform reads where the value is consumed, no b loads.
// ===========================================================================
#define HXP_BATCH 8   // (the specification record HxPairSpec: hx_post_abi.h)

template <bool BVEC>
__device__ __forceinline__ void hxp_load(const double *colA, const double *colB, int npad, int r, int last,
                                         double (&xa)[HXP_BATCH], double (&xb)[HXP_BATCH]) {
#pragma unroll
  for (int e = 0; e < HXP_BATCH; ++e) {
    const size_t off = (size_t)(r + e < last ? r + e : last) * (size_t)npad;
    xa[e] = colA[off];
    if (!BVEC) xb[e] = colB[off];
  }
}

// s = 0.0; s = s + x_y over the rows r0..r1 of one column, ascending; bad: a NaN among them
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__device__ __forceinline__ double hxp_row_sum(const double *col, int npad, int r0, int r1, unsigned &bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double xa[HXP_BATCH], xn[HXP_BATCH], unused[HXP_BATCH];
  double s = 0.0;
  hxp_load<true>(col, nullptr, npad, r0, r1, xa, unused);
  for (int r = r0; r <= r1; r += HXP_BATCH) {
    const bool more = r + HXP_BATCH <= r1;
    if (more) hxp_load<true>(col, nullptr, npad, r + HXP_BATCH, r1, xn, unused);
#pragma unroll
    for (int e = 0; e < HXP_BATCH; ++e) {
      if (r + e > r1) continue;   // wave-uniform
      s = s + xa[e];
      bad |= xa[e] != xa[e] ? 1u : 0u;
    }
    if (more) {
#pragma unroll
      for (int e = 0; e < HXP_BATCH; ++e) xa[e] = xn[e];
    }
  }
  return s;
}

// out[blockIdx.y][npad] in lane order; lanes >= n are not written
template <bool BVEC>
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_pair_metric_kernel(const double *__restrict__ va,
                                                             const double *__restrict__ vb,
                                                             const double *__restrict__ bvec, int bvec_iy0,
                                                             int n, int npad,
                                                             const HxPairSpec *__restrict__ specs,
                                                             double *__restrict__ out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= n) return;
  const HxPairSpec &sp = specs[blockIdx.y];
  const int op = sp.op, iy0 = sp.iy0, iy1 = sp.iy1;
  const double thr = sp.thr;
  const double *colA = va + lane;
  const double *colB = BVEC ? nullptr : vb + lane;
  unsigned bad = 0u;
  // the reference means; +0.0 without a reference period (x - 0.0 is x, bit for bit)
  double base_a = 0.0, base_b = 0.0;
  if (sp.a0 <= sp.a1) base_a = hxp_row_sum(colA, npad, sp.a0, sp.a1, bad) / (double)(sp.a1 - sp.a0 + 1);
  if (sp.b0 <= sp.b1) {
    double s = 0.0;
    if (BVEC) {
      for (int y = sp.b0; y <= sp.b1; ++y) s = s + bvec[y - bvec_iy0];
    } else {
      s = hxp_row_sum(colB, npad, sp.b0, sp.b1, bad);
    }
    base_b = s / (double)(sp.b1 - sp.b0 + 1);
  }
  double v;
  if (op == HX_PMET_END_RATIO) {
    const double xa0 = colA[(size_t)iy0 * (size_t)npad], xa1 = colA[(size_t)iy1 * (size_t)npad];
    const double xb0 = BVEC ? bvec[iy0 - bvec_iy0] : colB[(size_t)iy0 * (size_t)npad];
    const double xb1 = BVEC ? bvec[iy1 - bvec_iy0] : colB[(size_t)iy1 * (size_t)npad];
    bad |= (xa0 != xa0 || xa1 != xa1 || xb0 != xb0 || xb1 != xb1) ? 1u : 0u;
    const double a0 = xa0 - base_a, a1 = xa1 - base_a, b0 = xb0 - base_b, b1 = xb1 - base_b;
    const double da = a1 - a0, db = b1 - b0;
    v = da / db;
  } else {
    const bool regress = op == HX_PMET_SLOPE || op == HX_PMET_INTERCEPT || op == HX_PMET_R2;
    const bool negate = op == HX_PMET_AT_MAX;   // the largest b as the smallest -b: negation is exact
    const double nyears = (double)(iy1 - iy0 + 1);
    double xa[HXP_BATCH], xb[HXP_BATCH], na[HXP_BATCH], nb[HXP_BATCH];
    // pass 1.  acc / aux: sa, sb (regression); the reported a and found flag (AT_FIRST_GE); the reported
    // a and the extreme b (AT_MAX / AT_MIN); the sum and the count (MEAN_WHERE_GE)
    double acc = op == HX_PMET_AT_FIRST_GE ? __builtin_nan("") : 0.0, aux = 0.0;
    bool found = false;
    hxp_load<BVEC>(colA, colB, npad, iy0, iy1, xa, xb);
    for (int r = iy0; r <= iy1; r += HXP_BATCH) {
      const bool more = r + HXP_BATCH <= iy1;
      if (more) hxp_load<BVEC>(colA, colB, npad, r + HXP_BATCH, iy1, na, nb);   // in flight while this batch is consumed
#pragma unroll
      for (int e = 0; e < HXP_BATCH; ++e) {
        if (r + e > iy1) continue;   // wave-uniform
        const double rb = BVEC ? bvec[r + e - bvec_iy0] : xb[e];
        bad |= (xa[e] != xa[e] || rb != rb) ? 1u : 0u;
        const double a = xa[e] - base_a, b = rb - base_b;
        if (regress) {
          acc = acc + a;
          aux = aux + b;
        } else if (op == HX_PMET_AT_FIRST_GE) {
          if (!found && b >= thr) { acc = a; found = true; }
        } else if (op == HX_PMET_MEAN_WHERE_GE) {
          if (b >= thr) { acc = acc + a; aux = aux + 1.0; }
        } else {
          const double c = negate ? -b : b;
          if (r + e == iy0 || c < aux) { aux = c; acc = a; }
        }
      }
      if (more) {
#pragma unroll
        for (int e = 0; e < HXP_BATCH; ++e) { xa[e] = na[e]; if (!BVEC) xb[e] = nb[e]; }
      }
    }
    if (regress) {
      const double ma = acc / nyears, mb = aux / nyears;
      double sab = 0.0, sbb = 0.0, saa = 0.0;
      hxp_load<BVEC>(colA, colB, npad, iy0, iy1, xa, xb);
      for (int r = iy0; r <= iy1; r += HXP_BATCH) {
        const bool more = r + HXP_BATCH <= iy1;
        if (more) hxp_load<BVEC>(colA, colB, npad, r + HXP_BATCH, iy1, na, nb);
#pragma unroll
        for (int e = 0; e < HXP_BATCH; ++e) {
          if (r + e > iy1) continue;
          const double rb = BVEC ? bvec[r + e - bvec_iy0] : xb[e];
          const double a = xa[e] - base_a, b = rb - base_b;
          const double da = a - ma, db = b - mb;
          const double pab = db * da, pbb = db * db, paa = da * da;
          sab = sab + pab;
          sbb = sbb + pbb;
          saa = saa + paa;
        }
        if (more) {
#pragma unroll
          for (int e = 0; e < HXP_BATCH; ++e) { xa[e] = na[e]; if (!BVEC) xb[e] = nb[e]; }
        }
      }
      const double slope = sab / sbb;
      if (op == HX_PMET_SLOPE) {
        v = slope;
      } else if (op == HX_PMET_INTERCEPT) {
        const double p = slope * mb;
        v = ma - p;
      } else {
        const double num = sab * sab, den = sbb * saa;
        v = num / den;
      }
    } else if (op == HX_PMET_MEAN_WHERE_GE) {
      v = acc / aux;
    } else {
      v = acc;
    }
  }
  if (bad) v = __builtin_nan("");
  out[(size_t)blockIdx.y * (size_t)npad + (size_t)lane] = v;
}

// b: a [rows][npad] block in lane order, or nullptr with bvec[iy - bvec_iy0] on the device
hipError_t hx_launch_pair_metric(const double *a, const double *b, const double *bvec, int bvec_iy0, int n,
                                 int npad, const void *specs, int nspecs, double *out, hipStream_t st) {
  const dim3 grid((n + 255) / 256, nspecs), block(256);
  if (b)
    hipLaunchKernelGGL(hx_pair_metric_kernel<false>, grid, block, 0, st, a, b, bvec, bvec_iy0, n, npad,
                       (const HxPairSpec *)specs, out);
  else
    hipLaunchKernelGGL(hx_pair_metric_kernel<true>, grid, block, 0, st, a, b, bvec, bvec_iy0, n, npad,
                       (const HxPairSpec *)specs, out);
  return hipGetLastError();
}

#ifndef HX_HOST_EMULATION
// ===========================================================================
// Weighted quantiles (inverted CDF, Hyndman-Fan type 1) of a year row by an exact radix select.
//
// key(x): the order-preserving 64-bit image of a double (sign-flip transform); weights are the
// integers q (hx_fleet.cpp quantises them once), so every histogram is an exact integer sum and the
// answer -- a key some member has -- does not depend on lane order, shard split or summation order.
//
// Per year the select keeps `lo`: the bits >= lo of the answer are known (prefix[year][prob], zero
// below lo); 0 = finished.  It starts at the highest bit in which the row's min and max keys differ
// (hx_q_minmax_kernel + hx_q_init_kernel): the rows of a climate ensemble are tightly clustered and
// the leading digits carry no information.  A pass (hx_q_hist_kernel) reads the row ONCE for all
// probabilities, takes the 8-bit digit below lo of every key that matches a probability's prefix
// and adds its weight to that probability's 256-bin histogram in LDS (64-bit ds_add); probabilities
// whose prefixes still agree share one histogram.  hx_q_pick_kernel walks the histogram to the bin
// that holds the target rank, extends the prefix by it and clears the histogram for the next pass.
// ===========================================================================
#define HXQ_BLOCK 256
#define HXQ_PER 32       // keys of a row per lane: in registers during a histogram pass
#define HXQ_CHUNK (HXQ_BLOCK * HXQ_PER)  // elements of a row per workgroup
// (HXQ_MAXP, hxq_u64 and the year record HxQYear: hx_post_abi.h)

__device__ __forceinline__ hxq_u64 hxq_key(double x) {
  const hxq_u64 b = (hxq_u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// st[year] must be zero on entry (kmin is kept complemented so that zero is the identity of max)
__global__ __launch_bounds__(HXQ_BLOCK) void hx_q_minmax_kernel(const double *var, int n, int npad,
                                                                int iy0, const hxq_u64 *q, HxQYear *st) {
  const double *row = var + (size_t)(iy0 + (int)blockIdx.y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  hxq_u64 nkmin = 0, kmax = 0, W = 0, cnt = 0;
  for (int i = beg + (int)threadIdx.x; i < end; i += HXQ_BLOCK) {
    const double x = row[i];
    const hxq_u64 w = q ? q[i] : 1ull;
    if (x == x && w) {
      const hxq_u64 k = hxq_key(x);
      nkmin = max(nkmin, ~k); kmax = max(kmax, k); W += w; ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nkmin = max(nkmin, __shfl_down(nkmin, off, 64)); kmax = max(kmax, __shfl_down(kmax, off, 64));
    W += __shfl_down(W, off, 64); cnt += __shfl_down(cnt, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    HxQYear *o = st + blockIdx.y;
    atomicMax(&o->nkmin, nkmin); atomicMax(&o->kmax, kmax); atomicAdd(&o->W, W); atomicAdd(&o->cnt, cnt);
  }
}

// rank of the probs[j]-quantile among W units of weight: max(1, ceil(p * W)); W <= 2^52 is exact
__host__ __device__ inline hxq_u64 hxq_target(double p, hxq_u64 W) {
  const double t = ceil(p * (double)W);
  return t < 1.0 ? 1ull : (hxq_u64)t;
}
// where the select of a year starts: -> lo, *pre = the bits the row's keys have in common
__host__ __device__ inline int hxq_start(const HxQYear &s, int skip, hxq_u64 *pre) {
  *pre = 0;
  if (s.cnt == 0) return 0;
  if (!skip) return 64;
  const hxq_u64 kmin = ~s.nkmin, diff = kmin ^ s.kmax;
  if (!diff) { *pre = kmin; return 0; }
  int lo = 0;
  while (lo < 64 && (diff >> lo)) ++lo;   // highest differing bit + 1
  if (lo < 64) *pre = (kmin >> lo) << lo;
  return lo;
}

__global__ __launch_bounds__(64) void hx_q_init_kernel(const HxQYear *st, int ny, const double *probs,
                                                       int np, int skip, int *lo, hxq_u64 *prefix,
                                                       hxq_u64 *rem) {
  const int y = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (y >= ny) return;
  const HxQYear s = st[y];
  hxq_u64 pre;
  lo[y] = hxq_start(s, skip, &pre);
  for (int j = 0; j < np; ++j) {
    prefix[(size_t)y * np + j] = pre;
    rem[(size_t)y * np + j] = hxq_target(probs[j], s.W);
  }
}

// adds w to h[bin] for the lanes with `on`; the whole wavefront calls it together.  aggregate: the
// lanes that hit the bin of the first active lane are folded into one atomic (a popcount without
// weights), twice, then whoever is left adds on its own.  Measured (profiles/post_summaries.md):
// once the select starts below the common prefix the digits are spread out and the two ballots cost
// more than the contention they avoid (1.08 against 0.85 ms), so the host passes 0; the arm
// stays for rows that sit in two or three bins and for the next measurement.
__device__ __forceinline__ void hxq_add(hxq_u64 *h, int bin, hxq_u64 w, bool on, bool weighted,
                                        bool aggregate, int lane) {
  if (aggregate) {
    hxq_u64 todo = __ballot(on);
    for (int it = 0; it < 2 && todo; ++it) {
      const int leader = __ffsll((long long)todo) - 1;
      const int b = __shfl(bin, leader, 64);
      const bool mine = on && bin == b;
      const hxq_u64 m = __ballot(mine);
      hxq_u64 s;
      if (!weighted) {
        s = (hxq_u64)__popcll(m);
      } else {
        s = mine ? w : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      }
      if (lane == leader) atomicAdd(h + b, s);
      todo &= ~m;
      if (mine) on = false;
    }
  }
  if (on) atomicAdd(h + bin, w);
}

// grid (row chunks, years); hist[year][prob][256] accumulates over the chunks (and is cleared by
// hx_q_pick_kernel, or by the host between the passes of a sharded core).  A lane takes its
// HXQ_PER keys of the chunk into registers first -- every load of the lane in flight at once, the
// row read once -- and then goes through the probabilities with the prefix in scalar registers.
template <bool WEIGHTED>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_q_hist_kernel(const double *var, int n, int npad,
                                                              int iy0, const hxq_u64 *q, const int *lo,
                                                              const hxq_u64 *prefix, int np,
                                                              int aggregate, hxq_u64 *hist) {
  __shared__ hxq_u64 h[HXQ_MAXP * 256];
  __shared__ hxq_u64 pre[HXQ_MAXP];
  __shared__ int own[HXQ_MAXP];   // 1: this probability fills a histogram; 0: an earlier one with the same prefix does
  const int y = (int)blockIdx.y;
  const int l = lo[y];
  if (l == 0) return;   // this year is finished (the same for the whole workgroup)
  const int shift = l >= 8 ? l - 8 : 0;
  const hxq_u64 known = l >= 64 ? 0ull : ~0ull << l;   // the bits of a key that must equal the prefix
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  hxq_u64 k[HXQ_PER], w[WEIGHTED ? HXQ_PER : 1];
  unsigned part = 0;   // bit e: key e is a member's and not NaN
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const int i = beg + e * HXQ_BLOCK + tid;
    double x = __builtin_nan("");
    if (i < end) x = row[i];
    if (WEIGHTED) w[e] = i < end ? q[i] : 0ull;   // (a weight of zero adds nothing)
    k[e] = hxq_key(x);
    part |= (x == x ? 1u : 0u) << e;
  }
  if (tid < np) pre[tid] = prefix[(size_t)y * np + tid];
  for (int i = tid; i < np * 256; i += HXQ_BLOCK) h[i] = 0;
  __syncthreads();
  if (tid < np) {
    int o = 1;
    for (int c = 0; c < tid; ++c) if (pre[c] == pre[tid]) { o = 0; break; }
    own[tid] = o;
  }
  __syncthreads();
  for (int j = 0; j < np; ++j) {
    if (!own[j]) continue;
    const hxq_u64 p = pre[j];
    hxq_u64 *hj = h + j * 256;
#pragma unroll
    for (int e = 0; e < HXQ_PER; ++e) {
      const bool on = ((part >> e) & 1u) && ((k[e] ^ p) & known) == 0;
      const int digit = (int)((k[e] >> shift) & 255ull);
      hxq_add(hj, digit, WEIGHTED ? w[e] : 1ull, on, WEIGHTED, aggregate != 0, lane);
    }
  }
  __syncthreads();
  hxq_u64 *g = hist + (size_t)y * np * 256;
  for (int i = tid; i < np * 256; i += HXQ_BLOCK) {
    const hxq_u64 v = h[i];
    if (v) atomicAdd(g + i, v);
  }
}

// One workgroup per year, one wavefront per probability: the bin in which the running sum of the
// histogram reaches the remaining rank -> prefix extended, rank made relative to that bin, lo
// lowered, histogram cleared.
__global__ __launch_bounds__(64 * HXQ_MAXP) void hx_q_pick_kernel(int *lo, hxq_u64 *prefix, hxq_u64 *rem,
                                                                 int np, hxq_u64 *hist) {
  __shared__ hxq_u64 pre[HXQ_MAXP];
  const int y = (int)blockIdx.x;
  const int l = lo[y];
  if (l == 0) return;
  const int shift = l >= 8 ? l - 8 : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, j = tid >> 6;
  if (tid < np) pre[tid] = prefix[(size_t)y * np + tid];
  __syncthreads();
  int a = j;
  for (int k = 0; k < j; ++k) if (pre[k] == pre[j]) { a = k; break; }
  hxq_u64 *g = hist + (size_t)y * np * 256;
  const hxq_u64 *hh = g + (size_t)a * 256 + lane * 4;
  const hxq_u64 c0 = hh[0], c1 = hh[1], c2 = hh[2], c3 = hh[3];
  const hxq_u64 s = c0 + c1 + c2 + c3;
  hxq_u64 incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const hxq_u64 v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const hxq_u64 t = rem[(size_t)y * np + j];
  const hxq_u64 hit = __ballot(incl >= t);
  const int first = hit ? __ffsll((long long)hit) - 1 : 63;
  if (lane == first) {
    hxq_u64 cum = incl - s;
    int b = 3;
    if (cum + c0 >= t) b = 0;
    else if (cum + c0 + c1 >= t) { b = 1; cum += c0; }
    else if (cum + c0 + c1 + c2 >= t) { b = 2; cum += c0 + c1; }
    else cum += c0 + c1 + c2;
    const hxq_u64 bin = (hxq_u64)(lane * 4 + b);
    prefix[(size_t)y * np + j] = (pre[j] & ~(255ull << shift)) | (bin << shift);
    rem[(size_t)y * np + j] = t - cum;
  }
  __syncthreads();   // every wavefront has read the histogram it shares
  for (int i = tid; i < np * 256; i += 64 * np) g[i] = 0;
  if (tid == 0) lo[y] = shift;
}

hipError_t hx_launch_q_minmax(const double *var, int n, int npad, int iy0, int ny,
                              const unsigned long long *q, void *st, hipStream_t stream) {
  hipLaunchKernelGGL(hx_q_minmax_kernel, dim3((n + HXQ_CHUNK - 1) / HXQ_CHUNK, ny), dim3(HXQ_BLOCK), 0,
                     stream, var, n, npad, iy0, q, (HxQYear *)st);
  return hipGetLastError();
}
hipError_t hx_launch_q_init(const void *st, int ny, const double *probs, int np, int skip, int *lo,
                            unsigned long long *prefix, unsigned long long *rem, hipStream_t stream) {
  hipLaunchKernelGGL(hx_q_init_kernel, dim3((ny + 63) / 64), dim3(64), 0, stream, (const HxQYear *)st, ny,
                     probs, np, skip, lo, prefix, rem);
  return hipGetLastError();
}
hipError_t hx_launch_q_hist(const double *var, int n, int npad, int iy0, int ny,
                            const unsigned long long *q, const int *lo, const unsigned long long *prefix,
                            int np, int aggregate, unsigned long long *hist, hipStream_t stream) {
  const dim3 grid((n + HXQ_CHUNK - 1) / HXQ_CHUNK, ny);
  if (q)
    hipLaunchKernelGGL(hx_q_hist_kernel<true>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, q, lo,
                       prefix, np, aggregate, hist);
  else
    hipLaunchKernelGGL(hx_q_hist_kernel<false>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, q, lo,
                       prefix, np, aggregate, hist);
  return hipGetLastError();
}
hipError_t hx_launch_q_pick(int ny, int *lo, unsigned long long *prefix, unsigned long long *rem, int np,
                            unsigned long long *hist, hipStream_t stream) {
  hipLaunchKernelGGL(hx_q_pick_kernel, dim3(ny), dim3(64 * np), 0, stream, lo, prefix, rem, np, hist);
  return hipGetLastError();
}

// ===========================================================================
// Weighted mid-ranks of a row's members and the CRPS of a row against an observation
// (hx_series_rank, hx_metric_ranks, hx_ensemble_crps in hector_amd.h) by a stable least-significant-
// digit radix sort of the row's (key, lane) pairs, 8 bits a pass.
//
// One workgroup of HXR_BLOCK threads per row; nothing is scanned or synchronised across workgroups,
// every sum that reaches a result is an integer or a fixed-shape tree of doubles.  The steps of a row:
//   gather  the row's lanes 0..n-1 in chunks of HXR_BLOCK: x is canonicalised (-0.0 -> +0.0) before
//           hxq_key, the members taking part (not NaN; the CRPS: and q > 0) are compacted in lane
//           order into (key, lane) buffer A, and min key, max key, W = sum q, the observation's sums
//           and the histogram of digit 0 are taken on the way.  Padding lanes (>= n) are never read.
//   sort    digits 0 .. hb / 8 only, hb the highest bit in which min and max key differ: the keys
//           share every bit above hb, so a row of equal values runs no pass.  A pass walks its source
//           in chunks of HXR_CHUNK, in order; a wavefront takes HXR_PER x 64 consecutive elements, 64
//           at a time: the lanes that hold the same digit are found with eight ballots (hxr_match),
//           the first of them adds their number to the wavefront's counter of that digit in LDS
//           (32-bit ds_add, its return value is the digit's count so far) and a lane's place within
//           its digit follows from the lanes below it.  One thread per digit then turns the
//           wavefronts' counters into offsets, running over the chunks, and the pairs are scattered
//           to the other buffer.  The histogram of the next digit is taken during the scatter.
//   ranks   forward over the sorted pairs: the running uint64 sum of q (shuffle scans as in
//           hx_q_pick_kernel, the wavefronts added in order) and the first index of every run of equal
//           keys go to the buffers the sort no longer needs; backward: the running sum at the end of
//           a run is the suffix minimum over the run ends, N = (sum before the run) + (sum at its end)
//           = 2 L + E, and z goes to the member's lane of the destination row.
//   CRPS    forward with the same running sum: one thread per boundary between two runs evaluates
//           the terms of hector_amd.h, a thread adds its terms in chunk order, the threads are added
//           by a shuffle tree per wavefront and the wavefronts in order.
// Scratch per row: two key and two lane buffers of n entries (hx_rank_row_words); the host runs the
// rows in batches that keep it under HXR_SCRATCH_BYTES.  Every scatter is held to the row's count
// and every lane read back from a buffer to n before it is used as an index.
// ===========================================================================
#define HXR_BLOCK 512
#define HXR_WAVES (HXR_BLOCK / 64)
#define HXR_PER 4
#define HXR_CHUNK (HXR_BLOCK * HXR_PER)
#define HXR_MODE_CRPS 2   // modes 0 and 1 are HX_RANK_PIT and HX_RANK_NUMERATOR
static_assert(HX_RANK_PIT == 0 && HX_RANK_NUMERATOR == 1, "the header's kinds are the kernel's modes");
// (a row's result record HxRankOut: hx_post_abi.h)

__device__ __forceinline__ double hxr_unkey(hxq_u64 key) {
  const hxq_u64 b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)b);
}

// the lanes with `on` that hold the same digit as this one (called by the whole wavefront together)
__device__ __forceinline__ hxq_u64 hxr_match(int digit, bool on) {
  hxq_u64 m = __ballot(on);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1;
    const hxq_u64 v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

// the terms of one boundary between the runs a < b of the sorted row against the observation y:
// C = the running sum at the end of run a
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__device__ __forceinline__ double hxr_crps_terms(double acc, double a, double b, double y, hxq_u64 C, hxq_u64 W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double F = (double)C / (double)W, G = (double)(W - C) / (double)W;
  const double FF = F * F, GG = G * G;
  if (y <= a) {
    const double t = (b - a) * GG;
    acc = acc + t;
  } else if (y >= b) {
    const double t = (b - a) * FF;
    acc = acc + t;
  } else {
    const double t = (y - a) * FF, u = (b - y) * GG;
    acc = acc + t;
    acc = acc + u;
  }
  return acc;
}

// the sum of v over the workgroup in every thread: a shuffle tree per wavefront, the wavefronts in
// order (slot: HXR_WAVES words of LDS; two barriers)
__device__ __forceinline__ hxq_u64 hxr_block_sum(hxq_u64 v, hxq_u64 *slot, int lane, int wv) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if (lane == 0) slot[wv] = v;
  __syncthreads();
  hxq_u64 s = 0;
  for (int w = 0; w < HXR_WAVES; ++w) s += slot[w];
  return s;
}
__device__ __forceinline__ hxq_u64 hxr_block_max(hxq_u64 v, hxq_u64 *slot, int lane, int wv) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if (lane == 0) slot[wv] = v;
  __syncthreads();
  hxq_u64 s = 0;
  for (int w = 0; w < HXR_WAVES; ++w) s = max(s, slot[w]);
  return s;
}

// grid (rows); row r reads src row (rows ? rows[r] : row0 + r) and, for the rank modes, writes dst
// row dst_row0 + r (NaN on entry: a lane that takes no part keeps it); the CRPS writes res[r]
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(HXR_BLOCK) void hx_rank_kernel(const double *__restrict__ src, int n, int npad, int row0,
                                                            const int *__restrict__ rows,
                                                            const hxq_u64 *__restrict__ q, int mode,
                                                            const double *__restrict__ obs, hxq_u64 *scratch,
                                                            double *dst, int dst_row0, HxRankOut *res) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  __shared__ unsigned cnt[2][HXR_WAVES][256];
  __shared__ unsigned hist[2][256];
  __shared__ unsigned base[256];
  __shared__ hxq_u64 wtot[HXR_WAVES], wsec[HXR_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = (int)blockIdx.x;
  const bool crps = mode == HXR_MODE_CRPS;
  const double *row = src + (size_t)(rows ? rows[r] : row0 + r) * (size_t)npad;
  const size_t cap = ((size_t)n + 1) & ~(size_t)1;
  hxq_u64 *ksrc = scratch + (size_t)r * 3 * cap, *kdst = ksrc + cap;
  int *lsrc = reinterpret_cast<int *>(kdst + cap), *ldst = lsrc + cap;
  const hxq_u64 below = lane ? ~0ull >> (64 - lane) : 0ull;   // the lanes under this one

  double yobs = crps ? obs[r] : 0.0;
  if (yobs == 0.0) yobs = 0.0;
  if (crps && yobs != yobs) {   // (the same for the whole workgroup)
    if (tid == 0) { res[r].crps = __builtin_nan(""); res[r].pit = __builtin_nan(""); res[r].npart = 0; res[r].pad = 0; }
    return;
  }
  const hxq_u64 ky = hxq_key(yobs);

  // ---- gather ----------------------------------------------------------------------------------
  if (tid < 256) { hist[0][tid] = 0; hist[1][tid] = 0; }
  __syncthreads();
  hxq_u64 nkmin = 0, kmax = 0, W = 0, lt = 0, eq = 0;
  int m = 0;   // members gathered so far (the same in every thread)
  for (int cb = 0; cb < n; cb += HXR_BLOCK) {
    const int i = cb + tid;
    const bool in = i < n;
    double x = __builtin_nan("");
    if (in) x = row[i];
    if (x == 0.0) x = 0.0;
    const hxq_u64 w = (in && q) ? q[i] : 1ull;
    const bool part = in && x == x && (!crps || w != 0);
    const hxq_u64 k = hxq_key(x);
    if (part) {
      nkmin = max(nkmin, ~k); kmax = max(kmax, k); W += w;
      if (k < ky) lt += w;
      if (k == ky) eq += w;
    }
    const hxq_u64 pm = __ballot(part);
    if (lane == 0) wtot[wv] = (hxq_u64)__popcll(pm);
    const int d = (int)(k & 255ull);
    const hxq_u64 mm = hxr_match(d, part);
    if (part && lane == __ffsll((long long)mm) - 1) atomicAdd(&hist[0][d], (unsigned)__popcll(mm));
    __syncthreads();
    int off = m, tot = 0;
    for (int w2 = 0; w2 < HXR_WAVES; ++w2) {
      const int c = (int)wtot[w2];
      if (w2 < wv) off += c;
      tot += c;
    }
    if (part) {
      const int pos = off + __popcll(pm & below);
      if (pos < n) { ksrc[pos] = k; lsrc[pos] = i; }
    }
    m += tot;
    __syncthreads();
  }
  nkmin = hxr_block_max(nkmin, wtot, lane, wv);
  kmax = hxr_block_max(kmax, wsec, lane, wv);
  W = hxr_block_sum(W, wtot, lane, wv);
  lt = hxr_block_sum(lt, wsec, lane, wv);
  eq = hxr_block_sum(eq, wtot, lane, wv);
  __syncthreads();
  if (m == 0 || W == 0) {   // nobody takes part: the rank row stays NaN
    if (crps && tid == 0) { res[r].crps = __builtin_nan(""); res[r].pit = __builtin_nan(""); res[r].npart = 0; res[r].pad = 0; }
    return;
  }

  // ---- sort ------------------------------------------------------------------------------------
  const hxq_u64 diff = ~nkmin ^ kmax;
  const int npass = diff ? (63 - __clzll((long long)diff)) / 8 + 1 : 0;
  for (int p = 0; p < npass; ++p) {
    const int shift = 8 * p, hc = p & 1, hn = hc ^ 1;
    const bool next = p + 1 < npass;
    if (wv == 0) {   // base[d] = the keys with a smaller digit
      const unsigned c0 = hist[hc][4 * lane], c1 = hist[hc][4 * lane + 1], c2 = hist[hc][4 * lane + 2],
                     c3 = hist[hc][4 * lane + 3];
      const unsigned s = c0 + c1 + c2 + c3;
      unsigned incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      const unsigned ex = incl - s;
      base[4 * lane] = ex; base[4 * lane + 1] = ex + c0; base[4 * lane + 2] = ex + c0 + c1;
      base[4 * lane + 3] = ex + c0 + c1 + c2;
    }
    for (int j = lane; j < 256; j += 64) { cnt[0][wv][j] = 0; cnt[1][wv][j] = 0; }
    if (tid < 256) hist[hn][tid] = 0;   // (last read a pass ago, as that pass's hist[hc])
    __syncthreads();
    int buf = 0;
    for (int cb = 0; cb < m; cb += HXR_CHUNK, buf ^= 1) {
      hxq_u64 k[HXR_PER];
      int ln[HXR_PER];
      unsigned rk[HXR_PER];
#pragma unroll
      for (int e = 0; e < HXR_PER; ++e) {
        const int i = cb + wv * (64 * HXR_PER) + e * 64 + lane;
        k[e] = 0; ln[e] = 0;
        if (i < m) { k[e] = ksrc[i]; ln[e] = lsrc[i]; }
      }
#pragma unroll
      for (int e = 0; e < HXR_PER; ++e) {
        const int i = cb + wv * (64 * HXR_PER) + e * 64 + lane;
        const bool on = i < m;
        const int d = (int)((k[e] >> shift) & 255ull);
        const hxq_u64 mm = hxr_match(d, on);
        const int leader = on ? __ffsll((long long)mm) - 1 : lane;
        unsigned old = 0;
        if (on && lane == leader) old = atomicAdd(&cnt[buf][wv][d], (unsigned)__popcll(mm));
        old = __shfl(old, leader, 64);
        rk[e] = old + (unsigned)__popcll(mm & below);
        if (next) {
          const int d2 = (int)((k[e] >> (shift + 8)) & 255ull);
          const hxq_u64 m2 = hxr_match(d2, on);
          if (on && lane == __ffsll((long long)m2) - 1) atomicAdd(&hist[hn][d2], (unsigned)__popcll(m2));
        }
      }
      __syncthreads();
      if (tid < 256) {   // the wavefronts' counts of digit tid -> where each of them starts
        unsigned run = base[tid];
        for (int w2 = 0; w2 < HXR_WAVES; ++w2) {
          const unsigned c = cnt[buf][w2][tid];
          cnt[buf][w2][tid] = run;
          run += c;
        }
        base[tid] = run;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < HXR_PER; ++e) {
        const int i = cb + wv * (64 * HXR_PER) + e * 64 + lane;
        if (i < m) {
          const int d = (int)((k[e] >> shift) & 255ull);
          const unsigned pos = cnt[buf][wv][d] + rk[e];
          if (pos < (unsigned)m) { kdst[pos] = k[e]; ldst[pos] = ln[e]; }
        }
      }
      // this wavefront's counters of the next chunk (last read by it a chunk ago)
      for (int j = lane; j < 256; j += 64) cnt[buf ^ 1][wv][j] = 0;
    }
    __syncthreads();
    { hxq_u64 *t = ksrc; ksrc = kdst; kdst = t; }
    { int *t = lsrc; lsrc = ldst; ldst = t; }
  }

  const int nch = (m + HXR_BLOCK - 1) / HXR_BLOCK;
  if (crps) {
    // ---- CRPS --------------------------------------------------------------------------------
    hxq_u64 carry = 0;
    double acc = 0.0;
    if (tid == 0) {
      const double v1 = hxr_unkey(ksrc[0]), vm = hxr_unkey(ksrc[m - 1]);
      if (yobs < v1) acc = v1 - yobs;
      if (yobs > vm) acc = yobs - vm;
    }
    for (int c = 0; c < nch; ++c) {
      const int i = c * HXR_BLOCK + tid;
      const bool on = i < m;
      hxq_u64 k = 0, w = 0;
      if (on) {
        k = ksrc[i];
        const int l = lsrc[i];
        w = q ? ((unsigned)l < (unsigned)n ? q[l] : 0ull) : 1ull;
      }
      hxq_u64 incl = w;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const hxq_u64 v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[wv] = incl;
      __syncthreads();
      hxq_u64 off = carry, tot = 0;
      for (int w2 = 0; w2 < HXR_WAVES; ++w2) {
        const hxq_u64 t = wtot[w2];
        if (w2 < wv) off += t;
        tot += t;
      }
      carry += tot;
      if (on && i + 1 < m) {
        const hxq_u64 kn = ksrc[i + 1];
        if (kn != k) acc = hxr_crps_terms(acc, hxr_unkey(k), hxr_unkey(kn), yobs, off + incl, W);
      }
      __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_down(acc, o, 64);
    double *dsum = reinterpret_cast<double *>(wsec);
    if (lane == 0) dsum[wv] = acc;
    __syncthreads();
    if (tid == 0) {
      double s = dsum[0];
      for (int w2 = 1; w2 < HXR_WAVES; ++w2) s = s + dsum[w2];
      res[r].crps = s;
      res[r].pit = (double)(2 * lt + eq) / (double)(2 * W);
      res[r].npart = (long long)m;
      res[r].pad = 0;
    }
    return;
  }

  // ---- ranks, forward: kdst[i] = the running sum of q up to and including i, ldst[i] = the first
  // index of i's run ---------------------------------------------------------------------------
  {
    hxq_u64 carry = 0;
    int cstart = 0;
    for (int c = 0; c < nch; ++c) {
      const int i = c * HXR_BLOCK + tid;
      const bool on = i < m;
      hxq_u64 k = 0, w = 0;
      int st = 0;
      if (on) {
        k = ksrc[i];
        const int l = lsrc[i];
        w = q ? ((unsigned)l < (unsigned)n ? q[l] : 0ull) : 1ull;
        if (i > 0 && ksrc[i - 1] != k) st = i;
      }
      hxq_u64 incl = w;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const hxq_u64 v = __shfl_up(incl, o, 64);
        const int s2 = __shfl_up(st, o, 64);
        if (lane >= o) { incl += v; st = max(st, s2); }
      }
      if (lane == 63) { wtot[wv] = incl; wsec[wv] = (hxq_u64)st; }
      __syncthreads();
      hxq_u64 off = carry, tot = 0;
      int sbefore = cstart, sall = cstart;
      for (int w2 = 0; w2 < HXR_WAVES; ++w2) {
        const hxq_u64 t = wtot[w2];
        const int s2 = (int)wsec[w2];
        if (w2 < wv) { off += t; sbefore = max(sbefore, s2); }
        tot += t; sall = max(sall, s2);
      }
      carry += tot; cstart = sall;
      if (on) { kdst[i] = off + incl; ldst[i] = max(st, sbefore); }
      __syncthreads();
    }
  }
  // ---- ranks, backward: the running sum at the end of i's run is the smallest one over the run
  // ends at or after i -----------------------------------------------------------------------------
  {
    double *out = dst + (size_t)(dst_row0 + r) * (size_t)npad;
    const double twoW = (double)(2 * W);
    hxq_u64 carry = ~0ull;
    for (int c = nch - 1; c >= 0; --c) {
      const int i = c * HXR_BLOCK + tid;
      const bool on = i < m;
      hxq_u64 v = ~0ull;
      if (on && (i == m - 1 || ksrc[i + 1] != ksrc[i])) v = kdst[i];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const hxq_u64 t = __shfl_down(v, o, 64);
        if (lane + o < 64) v = min(v, t);
      }
      if (lane == 0) wtot[wv] = v;
      __syncthreads();
      hxq_u64 after = carry, all = carry;
      for (int w2 = 0; w2 < HXR_WAVES; ++w2) {
        const hxq_u64 t = wtot[w2];
        if (w2 > wv) after = min(after, t);
        all = min(all, t);
      }
      carry = all;
      if (on) {
        const hxq_u64 H = min(v, after);
        const int st = ldst[i], l = lsrc[i];
        const hxq_u64 L = (st > 0 && st <= i) ? kdst[st - 1] : 0ull;
        const hxq_u64 N = L + H;
        const double z = mode == HX_RANK_NUMERATOR ? (double)N : (double)N / twoW;
        if ((unsigned)l < (unsigned)n) out[l] = z;
      }
      __syncthreads();
    }
  }
}

// 8-byte words of scratch a row of n members needs; the most scratch a batch of rows may take
size_t hx_rank_row_words(int n) { return 3 * (((size_t)n + 1) & ~(size_t)1); }
#define HXR_SCRATCH_BYTES ((size_t)HX_RANK_SCRATCH_MIB << 20)
size_t hx_rank_scratch_bytes() { return HXR_SCRATCH_BYTES; }
hipError_t hx_launch_rank(const double *src, int n, int npad, int row0, const int *rows, int nrows,
                          const unsigned long long *q, int mode, const double *obs, unsigned long long *scratch,
                          double *dst, int dst_row0, void *res, hipStream_t stream) {
  hipLaunchKernelGGL(hx_rank_kernel, dim3(nrows), dim3(HXR_BLOCK), 0, stream, src, n, npad, row0, rows, q, mode,
                     obs, scratch, dst, dst_row0, (HxRankOut *)res);
  return hipGetLastError();
}

// ===========================================================================
// Weighted bin sums of rows against fixed edges (hx_ensemble_probabilities, hx_metric_probabilities).
// grid (row chunks, rows) like hx_q_hist_kernel; a lane takes its HXQ_PER values of the chunk into
// registers first.  bin(x) = the number of edges <= x: a branch-free binary search over the edges in
// LDS (32 slots, the unused ones NaN: `edge <= x` is false for them, also for x = +inf).  There are
// at most 32 bins, so one histogram would put a wavefront's adds on a handful of addresses: the
// workgroup keeps HXB_COPIES histograms, h[bin][copy] with copy = thread & 31 -- the copies of a bin
// lie in different banks, an address is shared by eight threads -- adds with 64-bit ds_add, then
// sums the copies (rotated: conflict-free) and flushes each bin once.  sums[row][K + 2]: the K + 1
// bins, then the number of members that took part; zero on entry.
// ===========================================================================
#define HXB_COPIES 32
template <bool WEIGHTED>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_bin_kernel(const double *var, int n, int npad, int iy0,
                                                           const hxq_u64 *q, const double *edges, int K,
                                                           hxq_u64 *sums) {
  __shared__ hxq_u64 h[32 * HXB_COPIES];
  __shared__ double ed[32];
  __shared__ hxq_u64 hcnt;
  const int tid = (int)threadIdx.x;
  const double *row = var + (size_t)(iy0 + (int)blockIdx.y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  double x[HXQ_PER];
  hxq_u64 w[WEIGHTED ? HXQ_PER : 1];
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const int i = beg + e * HXQ_BLOCK + tid;
    x[e] = __builtin_nan("");
    if (i < end) x[e] = row[i];
    if (WEIGHTED) w[e] = i < end ? q[i] : 0ull;
  }
  if (tid < 32) ed[tid] = tid < K ? edges[tid] : __builtin_nan("");
  for (int i = tid; i < 32 * HXB_COPIES; i += HXQ_BLOCK) h[i] = 0;
  if (tid == 0) hcnt = 0;
  __syncthreads();
  const int copy = tid & (HXB_COPIES - 1);
  hxq_u64 cnt = 0;
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const double v = x[e];
    const hxq_u64 we = WEIGHTED ? w[e] : 1ull;
    int pos = 0;   // -> the number of edges <= v, 0..31 (slot 31 is never read)
#pragma unroll
    for (int step = 16; step > 0; step >>= 1)
      if (ed[pos + step - 1] <= v) pos += step;
    if (v == v && we) {
      atomicAdd(h + pos * HXB_COPIES + copy, we);
      ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((tid & 63) == 0 && cnt) atomicAdd(&hcnt, cnt);
  __syncthreads();
  hxq_u64 *g = sums + (size_t)blockIdx.y * (size_t)(K + 2);
  if (tid <= K) {
    hxq_u64 s = 0;
    for (int c = 0; c < HXB_COPIES; ++c) s += h[tid * HXB_COPIES + ((c + tid) & (HXB_COPIES - 1))];
    if (s) atomicAdd(g + tid, s);
  }
  if (tid == 0 && hcnt) atomicAdd(g + K + 1, hcnt);
}

hipError_t hx_launch_bin(const double *var, int n, int npad, int iy0, int nrows, const unsigned long long *q,
                         const double *edges, int K, unsigned long long *sums, hipStream_t stream) {
  const dim3 grid((n + HXQ_CHUNK - 1) / HXQ_CHUNK, nrows);
  if (q)
    hipLaunchKernelGGL(hx_bin_kernel<true>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, q, edges, K, sums);
  else
    hipLaunchKernelGGL(hx_bin_kernel<false>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, q, edges, K, sums);
  return hipGetLastError();
}

// ===========================================================================
// Weighted moments of rows and their cross moments with per-member predictors (hx_ensemble_moments,
// hx_metric_moments in hector_amd.h define the sums).  Three steps:
//   hx_mom_prepare_kernel  lane-local: the call's effective integer weights (the host has zeroed q
//                          where a predictor is not finite) and predictors arrive in member order
//                          and go to lane order; e_k = p_k - c_k (0 where q is 0, so that no NaN
//                          reaches a product)
//   hx_q_minmax_kernel     with that q: the row's smallest participating value c_y, W and the count
//   hx_moments_kernel<NP>  grid (row chunks, rows) like hx_q_hist_kernel: a lane takes its HXQ_PER
//                          values of the chunk into registers, a batch at a time with every load of
//                          the batch in flight -- the row is read once from memory; q and the
//                          predictors of the same members, which every row re-reads, come from the
//                          cache.  2 + 3 NP private accumulators, all terms >= 0.
// No floating atomics: a fixed shuffle tree per wavefront, the four wavefronts added in order, one
// partial per (row, chunk), and hx_mom_reduce_kernel adds the chunks in ascending order -- the same
// bits from call to call for one lane order and shard layout.
// ===========================================================================
#define HXMOM_MAXP 8
__global__ __launch_bounds__(256) void hx_mom_prepare_kernel(const hxq_u64 *__restrict__ q_mem,
                                                             const double *__restrict__ pred_mem, int npred,
                                                             int n, int npad,
                                                             const int *__restrict__ lane_of_member,
                                                             const double *__restrict__ c,
                                                             hxq_u64 *__restrict__ q_lane,
                                                             double *__restrict__ qd_lane,
                                                             double *__restrict__ e_lane) {
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= n) return;
  const int lane = lane_of_member[m];
  if (lane < 0 || lane >= npad) return;
  const hxq_u64 q = q_mem[m];   // (the host has zeroed it where a predictor is not finite)
  q_lane[lane] = q;
  qd_lane[lane] = (double)q;   // q <= 2^32: exact
  for (int k = 0; k < npred; ++k)
    e_lane[(size_t)k * (size_t)npad + (size_t)lane] = q ? pred_mem[(size_t)k * (size_t)n + (size_t)m] - c[k] : 0.0;
}

// part[(row * nchunks + chunk) * (2 + 3 NP) + ...] = A, B, then C_k, D_k, E_k of the chunk
template <int NP>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_moments_kernel(const double *__restrict__ var, int n, int npad,
                                                               int iy0, const double *__restrict__ qd,
                                                               const double *__restrict__ e,
                                                               const double *__restrict__ shift,
                                                               double *__restrict__ part) {
  constexpr int NC = 2 + 3 * NP;
  static_assert(HXQ_BLOCK == 256, "the combine below adds four wavefronts in a fixed order");
  __shared__ double red[HXQ_BLOCK / 64][NC];
  const int tid = (int)threadIdx.x;
  const int y = (int)blockIdx.y;
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  const double c = shift[y];
  double acc[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) acc[a] = 0.0;
  // HXQ_PER elements a lane in batches of B: the row values, weights and predictors of a batch are
  // all in flight at once; B shrinks with NP so that a batch and the accumulators stay in registers
  constexpr int B = NP == 0 ? HXQ_PER : NP <= 3 ? HXQ_PER / 2 : HXQ_PER / 4;
#pragma unroll 1
  for (int j0 = 0; j0 < HXQ_PER; j0 += B) {
    const int i0 = beg + j0 * HXQ_BLOCK + tid;
    if (i0 - tid >= end) break;   // (the same for the whole workgroup)
    double x[B], w[B], ek[NP > 0 ? NP * B : 1];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const int i = i0 + j * HXQ_BLOCK;
      const bool in = i < end;
      x[j] = __builtin_nan("");
      w[j] = 0.0;
      if (in) { x[j] = row[i]; w[j] = qd[i]; }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        ek[k * B + j] = 0.0;
        if (in) ek[k * B + j] = e[(size_t)k * (size_t)npad + (size_t)i];
      }
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const bool on = x[j] == x[j] && w[j] > 0.0;   // (on: somebody takes part, so c is a member's value)
      const double ww = on ? w[j] : 0.0;
      const double d = on ? x[j] - c : 0.0;
      const double wd = ww * d;
      acc[0] += wd;
      acc[1] += wd * d;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const double we = ww * ek[k * B + j];
        acc[2 + 3 * k] += we;
        acc[3 + 3 * k] += we * ek[k * B + j];
        acc[4 + 3 * k] += wd * ek[k * B + j];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    double v = acc[a];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6][a] = v;
  }
  __syncthreads();
  if (tid < NC)
    part[((size_t)y * gridDim.x + blockIdx.x) * NC + tid] =
        ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out[row][nc] = the chunks' partials added in ascending chunk order
__global__ __launch_bounds__(256) void hx_mom_reduce_kernel(const double *__restrict__ part, int nchunks, int nc,
                                                            int total, double *__restrict__ out) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (idx >= total) return;
  const int y = idx / nc, a = idx - y * nc;
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s += part[((size_t)y * nchunks + ch) * nc + a];
  out[idx] = s;
}

hipError_t hx_launch_mom_prepare(const unsigned long long *q_mem, const double *pred_mem, int npred, int n,
                                 int npad, const int *lane_of_member, const double *c,
                                 unsigned long long *q_lane, double *qd_lane, double *e_lane, hipStream_t st) {
  hipLaunchKernelGGL(hx_mom_prepare_kernel, dim3((n + 255) / 256), dim3(256), 0, st, q_mem, pred_mem, npred, n,
                     npad, lane_of_member, c, q_lane, qd_lane, e_lane);
  return hipGetLastError();
}
int hx_mom_chunks(int n) { return (n + HXQ_CHUNK - 1) / HXQ_CHUNK; }
// part: [nrows][hx_mom_chunks(n)][2 + 3 npred] scratch; out: [nrows][2 + 3 npred]
hipError_t hx_launch_moments(const double *var, int n, int npad, int iy0, int nrows, const double *qd,
                             const double *e, int npred, const double *shift, double *part, double *out,
                             hipStream_t st) {
  const int nchunks = hx_mom_chunks(n), nc = 2 + 3 * npred;
  const dim3 grid(nchunks, nrows), block(HXQ_BLOCK);
#define HXMOM_CASE(NP) \
  case NP: hipLaunchKernelGGL(hx_moments_kernel<NP>, grid, block, 0, st, var, n, npad, iy0, qd, e, shift, part); break;
  switch (npred) {
    HXMOM_CASE(0) HXMOM_CASE(1) HXMOM_CASE(2) HXMOM_CASE(3) HXMOM_CASE(4)
    HXMOM_CASE(5) HXMOM_CASE(6) HXMOM_CASE(7) HXMOM_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef HXMOM_CASE
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = nrows * nc;
  hipLaunchKernelGGL(hx_mom_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, part, nchunks, nc, total,
                     out);
  return hipGetLastError();
}

// ===========================================================================
// The grouped flavours of the three summaries above (hx_group_quantiles, hx_group_probabilities,
// hx_group_moments in hector_amd.h): every member carries a label 0 .. G-1 (G <= HXG_MAX) or -1, "in
// no group", and one pass sequence answers for every group what G calls with masked weights would.
// Lane order is a cost-sorted permutation, so a group's members are scattered in a row whatever the
// caller's labels look like, and gathered 8-byte loads cost 3.8 times the streamed read of the same
// bytes (profiles/post_summaries.md, the Sobol section): the kernels stay streamed -- a lane takes
// its HXQ_PER values of the chunk into registers as above, the row is read ONCE per pass whatever G
// is, and the lanes' labels (like q, re-read per row from the cache) say where a value counts.
// Rows of the state arrays are (group, row) pairs, r = g * nrows + row, which is the group-major
// layout of the results: hx_q_init_kernel, hx_q_pick_kernel and hx_mom_reduce_kernel run unchanged
// over G * nrows rows.
//   hx_grp_prepare_kernel   lane-local: labels from member order to lane order (padding lanes -1)
//   hx_gmom_prepare_kernel  hx_mom_prepare_kernel with the labels and per-group predictor shifts
//   hx_gq_minmax_kernel     per (row, group): wavefront reduction per group present in the
//                           wavefront, combined in LDS, one global atomic per group present in the chunk
//   hx_gq_hist_kernel       keys, weights and labels (4 bits each) stay in registers while the (group,
//                           probability) slots go through the LDS histograms in batches of 64 slots
//                           x 256 bins; a key is compared only against the prefixes of its own group;
//                           groups finish at different digits and are skipped then
//   hx_gbin_kernel          h[group][bin][copy], fewer copies per bin as G grows, flushed once
//   hx_gmoments_kernel<NP>  inside a register batch the groups present in the wavefront (a ballot
//                           skips the absent ones) take turns: private sums over the lanes whose label
//                           matches, the fixed shuffle tree, added to the wavefront's slot in LDS in
//                           batch order; one partial per (row, group, chunk)
// ===========================================================================
#define HXG_MAX 16
static_assert(HXG_MAX == HX_GROUP_MAX, "the header's limit");

__global__ __launch_bounds__(256) void hx_grp_prepare_kernel(const int *__restrict__ lab_mem, int n, int npad,
                                                             const int *__restrict__ lane_of_member,
                                                             int *__restrict__ lab_lane) {
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= n) return;
  const int lane = lane_of_member[m];
  if (lane < 0 || lane >= npad) return;
  lab_lane[lane] = lab_mem[m];
}

// c[g * HXMOM_MAXP + k]: the predictor shifts of group g; q_mem is 0 where the label is -1
__global__ __launch_bounds__(256) void hx_gmom_prepare_kernel(const hxq_u64 *__restrict__ q_mem,
                                                              const double *__restrict__ pred_mem,
                                                              const int *__restrict__ lab_mem, int npred, int n,
                                                              int npad, const int *__restrict__ lane_of_member,
                                                              const double *__restrict__ c,
                                                              hxq_u64 *__restrict__ q_lane,
                                                              double *__restrict__ qd_lane,
                                                              double *__restrict__ e_lane,
                                                              int *__restrict__ lab_lane) {
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= n) return;
  const int lane = lane_of_member[m];
  if (lane < 0 || lane >= npad) return;
  const int g = lab_mem[m];
  const hxq_u64 q = g >= 0 ? q_mem[m] : 0ull;
  lab_lane[lane] = g;
  q_lane[lane] = q;
  qd_lane[lane] = (double)q;
  for (int k = 0; k < npred; ++k)
    e_lane[(size_t)k * (size_t)npad + (size_t)lane] =
        q ? pred_mem[(size_t)k * (size_t)n + (size_t)m] - c[g * HXMOM_MAXP + k] : 0.0;
}

// st[g * ny + year] must be zero on entry
template <bool WEIGHTED>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_gq_minmax_kernel(const double *var, int n, int npad, int iy0,
                                                                 int ny, const hxq_u64 *q, const int *lab, int G,
                                                                 HxQYear *st) {
  __shared__ hxq_u64 s[HXG_MAX * 4];
  const int tid = (int)threadIdx.x;
  const int y = (int)blockIdx.y;
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  if (tid < HXG_MAX * 4) s[tid] = 0;
  hxq_u64 k[HXQ_PER], w[WEIGHTED ? HXQ_PER : 1];
  int lb[HXQ_PER];   // -1: no member here, NaN, weight 0 or in no group
  unsigned gm = 0;   // the groups this lane holds
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const int i = beg + e * HXQ_BLOCK + tid;
    double x = __builtin_nan("");
    int g = -1;
    hxq_u64 we = 1ull;
    if (i < end) { x = row[i]; g = lab[i]; if (WEIGHTED) we = q[i]; }
    if (!(x == x) || !we || g >= G) g = -1;
    if (WEIGHTED) w[e] = we;
    k[e] = hxq_key(x);
    lb[e] = g;
    if (g >= 0) gm |= 1u << g;
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    if (!__ballot((gm >> g) & 1u)) continue;   // wave-uniform
    hxq_u64 nkmin = 0, kmax = 0, W = 0, cnt = 0;
#pragma unroll
    for (int e = 0; e < HXQ_PER; ++e)
      if (lb[e] == g) {
        nkmin = max(nkmin, ~k[e]); kmax = max(kmax, k[e]); W += WEIGHTED ? w[e] : 1ull; ++cnt;
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      nkmin = max(nkmin, __shfl_down(nkmin, off, 64)); kmax = max(kmax, __shfl_down(kmax, off, 64));
      W += __shfl_down(W, off, 64); cnt += __shfl_down(cnt, off, 64);
    }
    if ((tid & 63) == 0) {
      atomicMax(&s[g * 4], nkmin); atomicMax(&s[g * 4 + 1], kmax);
      atomicAdd(&s[g * 4 + 2], W); atomicAdd(&s[g * 4 + 3], cnt);
    }
  }
  __syncthreads();
  if (tid < G && s[tid * 4 + 3]) {
    HxQYear *o = st + (size_t)tid * ny + y;
    atomicMax(&o->nkmin, s[tid * 4]); atomicMax(&o->kmax, s[tid * 4 + 1]);
    atomicAdd(&o->W, s[tid * 4 + 2]); atomicAdd(&o->cnt, s[tid * 4 + 3]);
  }
}

// grid (row chunks, years); lo[g * ny + year], prefix[(g * ny + year) * np + j], hist likewise x 256.
// Slot s = g * np + j.  The histograms of HXGQ_SLOTS slots at a time live in LDS (128 of the CU's 160
// KiB; the kernel's registers allow one workgroup per CU anyway), the keys stay in registers across
// the batches, and a key goes through the np prefixes of ITS group only: the work per key is that of
// the ungrouped kernel whatever G is.  Groups finish at different digits: every key takes the digit
// below the lo of its own group.
#define HXGQ_SLOTS 64
template <bool WEIGHTED>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_gq_hist_kernel(const double *var, int n, int npad, int iy0,
                                                               int ny, const hxq_u64 *q, const int *lab, int G,
                                                               const int *lo, const hxq_u64 *prefix, int np,
                                                               hxq_u64 *hist) {
  __shared__ hxq_u64 h[HXGQ_SLOTS * 256];
  __shared__ hxq_u64 pre[HXG_MAX * HXQ_MAXP];
  __shared__ int own[HXG_MAX * HXQ_MAXP];   // 1: this slot fills a histogram; 0: finished, or an earlier
                                            // probability of the group with the same prefix does
  __shared__ int glo[HXG_MAX];
  const int y = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const int S = G * np;   // <= 256 = HXQ_BLOCK
  if (tid < HXG_MAX) glo[tid] = tid < G ? lo[(size_t)tid * ny + y] : 0;
  if (tid < S) pre[tid] = prefix[((size_t)(tid / np) * ny + y) * np + (tid % np)];
  __syncthreads();
  bool open = false;
  for (int g = 0; g < G; ++g) open = open || glo[g] != 0;
  if (!open) return;   // every group of this year is finished (the same for the whole workgroup)
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  hxq_u64 k[HXQ_PER], w[WEIGHTED ? HXQ_PER : 1];
  unsigned part = 0;            // bit e: key e is a member's, not NaN, and in a group
  unsigned lab4[HXQ_PER / 8];   // its label, 4 bits each
#pragma unroll
  for (int e = 0; e < HXQ_PER / 8; ++e) lab4[e] = 0u;
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const int i = beg + e * HXQ_BLOCK + tid;
    double x = __builtin_nan("");
    int g = -1;
    if (i < end) { x = row[i]; g = lab[i]; }
    if (WEIGHTED) w[e] = i < end ? q[i] : 0ull;
    k[e] = hxq_key(x);
    const bool on = x == x && g >= 0 && g < G;
    part |= (on ? 1u : 0u) << e;
    lab4[e >> 3] |= (on ? (unsigned)g : 0u) << ((e & 7) * 4);
  }
  if (tid < S) {
    const int g = tid / np, j = tid - g * np;
    int o = glo[g] != 0 ? 1 : 0;
    for (int c = 0; c < j; ++c) if (pre[g * np + c] == pre[tid]) { o = 0; break; }
    own[tid] = o;
  }
  // keys of groups that have finished take no part in this pass
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e)
    if (glo[(lab4[e >> 3] >> ((e & 7) * 4)) & 15u] == 0) part &= ~(1u << e);
#pragma unroll 1
  for (int b0 = 0; b0 < S; b0 += HXGQ_SLOTS) {
    const int nb = min(HXGQ_SLOTS, S - b0);
    for (int i = tid; i < nb * 256; i += HXQ_BLOCK) h[i] = 0;
    __syncthreads();   // (the first time round: own[] is complete too)
    // (opaque to the optimiser: the 32 predicates below are then formed where they are used, one lane
    //  mask at a time, instead of being hoisted out of the batch loop into 64 scalar registers)
    unsigned pb = part;
    asm volatile("" : "+v"(pb));
#pragma unroll
    for (int e = 0; e < HXQ_PER; ++e) {
      const int g = (int)((lab4[e >> 3] >> ((e & 7) * 4)) & 15u);
      const int l = glo[g];
      const bool mine = ((pb >> e) & 1u) != 0;
      const int shift = l >= 8 ? l - 8 : 0;
      const hxq_u64 known = l >= 64 ? 0ull : ~0ull << l;
      const int digit = (int)((k[e] >> shift) & 255ull);
      const int s0 = g * np - b0;   // the group's first slot, relative to the batch
      for (int j = 0; j < np; ++j) {
        const int sl = s0 + j;
        const bool in = mine && sl >= 0 && sl < nb;
        const int s = in ? sl + b0 : 0;
        if (in && own[s] && ((k[e] ^ pre[s]) & known) == 0)
          atomicAdd(h + sl * 256 + digit, WEIGHTED ? w[e] : 1ull);
      }
    }
    __syncthreads();
    for (int i = tid; i < nb * 256; i += HXQ_BLOCK) {
      const hxq_u64 v = h[i];
      if (v) {
        const int s = b0 + (i >> 8), g = s / np;
        atomicAdd(hist + (((size_t)g * ny + y) * np + (s - g * np)) * 256 + (i & 255), v);
      }
    }
    __syncthreads();   // the histograms are cleared for the next batch
  }
}

// sums[(g * nrows + row)][K + 2]: the K + 1 bins, then the members that took part; zero on entry.
// Bin slot 32 of a group counts its members; C copies per bin: 32 up to four groups, 16 up to eight, 8
#define HXGB_WORDS (33 * 128)
template <bool WEIGHTED>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_gbin_kernel(const double *var, int n, int npad, int iy0, int nrows,
                                                            const hxq_u64 *q, const int *lab, int G,
                                                            const double *edges, int K, hxq_u64 *sums) {
  __shared__ hxq_u64 h[HXGB_WORDS];
  __shared__ double ed[32];
  const int tid = (int)threadIdx.x;
  const int y = (int)blockIdx.y;
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  const int C = G <= 4 ? 32 : G <= 8 ? 16 : 8;   // G * 33 * C <= HXGB_WORDS
  double x[HXQ_PER];
  hxq_u64 w[WEIGHTED ? HXQ_PER : 1];
  int lb[HXQ_PER];
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const int i = beg + e * HXQ_BLOCK + tid;
    x[e] = __builtin_nan("");
    lb[e] = -1;
    if (i < end) { x[e] = row[i]; lb[e] = lab[i]; }
    if (WEIGHTED) w[e] = i < end ? q[i] : 0ull;
  }
  if (tid < 32) ed[tid] = tid < K ? edges[tid] : __builtin_nan("");
  for (int i = tid; i < HXGB_WORDS; i += HXQ_BLOCK) h[i] = 0;
  __syncthreads();
  const int copy = tid & (C - 1);
#pragma unroll
  for (int e = 0; e < HXQ_PER; ++e) {
    const double v = x[e];
    const hxq_u64 we = WEIGHTED ? w[e] : 1ull;
    const int g = lb[e];
    int pos = 0;
#pragma unroll
    for (int step = 16; step > 0; step >>= 1)
      if (ed[pos + step - 1] <= v) pos += step;
    if (v == v && we && g >= 0 && g < G) {
      atomicAdd(h + (g * 33 + pos) * C + copy, we);
      atomicAdd(h + (g * 33 + 32) * C + copy, 1ull);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < G * (K + 2); idx += HXQ_BLOCK) {
    const int g = idx / (K + 2), b = idx - g * (K + 2);
    const hxq_u64 *hb = h + (g * 33 + (b <= K ? b : 32)) * C;
    hxq_u64 s = 0;
    for (int c = 0; c < C; ++c) s += hb[(c + idx) & (C - 1)];
    if (s) atomicAdd(sums + ((size_t)g * nrows + y) * (size_t)(K + 2) + b, s);
  }
}

// part[((g * nrows + row) * nchunks + chunk) * (2 + 3 NP) + ...]; shift[g * nrows + row]; e: the lane's
// predictors less the shifts of ITS group (hx_gmom_prepare_kernel); a group absent from the chunk
// writes zeros
template <int NP>
__global__ __launch_bounds__(HXQ_BLOCK) void hx_gmoments_kernel(const double *__restrict__ var, int n, int npad,
                                                                int iy0, int nrows, const double *__restrict__ qd,
                                                                const double *__restrict__ e,
                                                                const int *__restrict__ lab, int G,
                                                                const double *__restrict__ shift,
                                                                double *__restrict__ part) {
  constexpr int NC = 2 + 3 * NP;
  static_assert(HXQ_BLOCK == 256, "the combine below adds four wavefronts in a fixed order");
  __shared__ double red[HXQ_BLOCK / 64][HXG_MAX][NC];
  __shared__ double cg[HXG_MAX];
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  const int y = (int)blockIdx.y;
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = (int)blockIdx.x * HXQ_CHUNK, end = min(beg + HXQ_CHUNK, n);
  for (int i = tid; i < (HXQ_BLOCK / 64) * HXG_MAX * NC; i += HXQ_BLOCK) (&red[0][0][0])[i] = 0.0;
  if (tid < HXG_MAX) cg[tid] = tid < G ? shift[(size_t)tid * nrows + y] : 0.0;
  __syncthreads();
  // (batches of 16 up to one predictor, of 8 beyond: the labels and a group's accumulators share the
  //  registers with the batch, and the default code generation of the safe build must not spill either)
  constexpr int B = NP <= 1 ? HXQ_PER / 2 : HXQ_PER / 4;
#pragma unroll 1
  for (int j0 = 0; j0 < HXQ_PER; j0 += B) {
    const int i0 = beg + j0 * HXQ_BLOCK + tid;
    if (i0 - tid >= end) break;   // (the same for the whole workgroup)
    double x[B], w[B], ek[NP > 0 ? NP * B : 1];
    int lb[B];
    unsigned gm = 0;
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const int i = i0 + j * HXQ_BLOCK;
      const bool in = i < end;
      x[j] = __builtin_nan("");
      w[j] = 0.0;
      lb[j] = -1;
      if (in) { x[j] = row[i]; w[j] = qd[i]; lb[j] = lab[i]; }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        ek[k * B + j] = 0.0;
        if (in) ek[k * B + j] = e[(size_t)k * (size_t)npad + (size_t)i];
      }
      if (!(x[j] == x[j] && w[j] > 0.0) || lb[j] >= G) lb[j] = -1;   // takes no part
      if (lb[j] >= 0) gm |= 1u << lb[j];
    }
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      if (!__ballot((gm >> g) & 1u)) continue;   // wave-uniform: nobody of this group in the batch
      const double c = cg[g];
      double acc[NC];
#pragma unroll
      for (int a = 0; a < NC; ++a) acc[a] = 0.0;
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const bool on = lb[j] == g;
        const double ww = on ? w[j] : 0.0;
        const double d = on ? x[j] - c : 0.0;
        const double wd = ww * d;
        acc[0] += wd;
        acc[1] += wd * d;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const double we = ww * ek[k * B + j];
          acc[2 + 3 * k] += we;
          acc[3 + 3 * k] += we * ek[k * B + j];
          acc[4 + 3 * k] += wd * ek[k * B + j];
        }
      }
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        double v = acc[a];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[wave][g][a] += v;   // this wavefront's slot: batches in ascending order
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < G * NC; idx += HXQ_BLOCK) {
    const int g = idx / NC, a = idx - g * NC;
    part[(((size_t)g * nrows + y) * gridDim.x + blockIdx.x) * NC + a] =
        ((red[0][g][a] + red[1][g][a]) + red[2][g][a]) + red[3][g][a];
  }
}

hipError_t hx_launch_grp_prepare(const int *lab_mem, int n, int npad, const int *lane_of_member, int *lab_lane,
                                 hipStream_t st) {
  hipLaunchKernelGGL(hx_grp_prepare_kernel, dim3((n + 255) / 256), dim3(256), 0, st, lab_mem, n, npad,
                     lane_of_member, lab_lane);
  return hipGetLastError();
}
hipError_t hx_launch_gmom_prepare(const unsigned long long *q_mem, const double *pred_mem, const int *lab_mem,
                                  int npred, int n, int npad, const int *lane_of_member, const double *c,
                                  unsigned long long *q_lane, double *qd_lane, double *e_lane, int *lab_lane,
                                  hipStream_t st) {
  hipLaunchKernelGGL(hx_gmom_prepare_kernel, dim3((n + 255) / 256), dim3(256), 0, st, q_mem, pred_mem, lab_mem,
                     npred, n, npad, lane_of_member, c, q_lane, qd_lane, e_lane, lab_lane);
  return hipGetLastError();
}
hipError_t hx_launch_gq_minmax(const double *var, int n, int npad, int iy0, int ny, const unsigned long long *q,
                               const int *lab, int G, void *st, hipStream_t stream) {
  if (G < 1 || G > HXG_MAX) return hipErrorInvalidValue;
  const dim3 grid((n + HXQ_CHUNK - 1) / HXQ_CHUNK, ny);
  if (q)
    hipLaunchKernelGGL(hx_gq_minmax_kernel<true>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, ny, q, lab,
                       G, (HxQYear *)st);
  else
    hipLaunchKernelGGL(hx_gq_minmax_kernel<false>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, ny, q, lab,
                       G, (HxQYear *)st);
  return hipGetLastError();
}
hipError_t hx_launch_gq_hist(const double *var, int n, int npad, int iy0, int ny, const unsigned long long *q,
                             const int *lab, int G, const int *lo, const unsigned long long *prefix, int np,
                             unsigned long long *hist, hipStream_t stream) {
  if (G < 1 || G > HXG_MAX || np < 1 || np > HXQ_MAXP) return hipErrorInvalidValue;
  const dim3 grid((n + HXQ_CHUNK - 1) / HXQ_CHUNK, ny);
  if (q)
    hipLaunchKernelGGL(hx_gq_hist_kernel<true>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, ny, q, lab, G,
                       lo, prefix, np, hist);
  else
    hipLaunchKernelGGL(hx_gq_hist_kernel<false>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, ny, q, lab, G,
                       lo, prefix, np, hist);
  return hipGetLastError();
}
hipError_t hx_launch_gbin(const double *var, int n, int npad, int iy0, int nrows, const unsigned long long *q,
                          const int *lab, int G, const double *edges, int K, unsigned long long *sums,
                          hipStream_t stream) {
  if (G < 1 || G > HXG_MAX || K < 1 || K > 31) return hipErrorInvalidValue;
  const dim3 grid((n + HXQ_CHUNK - 1) / HXQ_CHUNK, nrows);
  if (q)
    hipLaunchKernelGGL(hx_gbin_kernel<true>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, nrows, q, lab, G,
                       edges, K, sums);
  else
    hipLaunchKernelGGL(hx_gbin_kernel<false>, grid, dim3(HXQ_BLOCK), 0, stream, var, n, npad, iy0, nrows, q, lab, G,
                       edges, K, sums);
  return hipGetLastError();
}
// part: [G][nrows][hx_mom_chunks(n)][2 + 3 npred] scratch; out: [G][nrows][2 + 3 npred]
hipError_t hx_launch_gmoments(const double *var, int n, int npad, int iy0, int nrows, const double *qd,
                              const double *e, const int *lab, int G, int npred, const double *shift,
                              double *part, double *out, hipStream_t st) {
  if (G < 1 || G > HXG_MAX) return hipErrorInvalidValue;
  const int nchunks = hx_mom_chunks(n), nc = 2 + 3 * npred;
  const dim3 grid(nchunks, nrows), block(HXQ_BLOCK);
#define HXGMOM_CASE(NP) \
  case NP: hipLaunchKernelGGL(hx_gmoments_kernel<NP>, grid, block, 0, st, var, n, npad, iy0, nrows, qd, e, lab, G, \
                              shift, part); break;
  switch (npred) {
    HXGMOM_CASE(0) HXGMOM_CASE(1) HXGMOM_CASE(2) HXGMOM_CASE(3) HXGMOM_CASE(4)
    HXGMOM_CASE(5) HXGMOM_CASE(6) HXGMOM_CASE(7) HXGMOM_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef HXGMOM_CASE
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = G * nrows * nc;
  hipLaunchKernelGGL(hx_mom_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, part, nchunks, nc, total,
                     out);
  return hipGetLastError();
}

// ===========================================================================
// Variance-based (Sobol) sensitivity sums from a Saltelli design (hx_ensemble_sobol, hx_metric_sobol
// in hector_amd.h define the sums).  The estimators compare members in matched groups -- member A_j
// with B_j and AB_i,j, k + 2 consecutive members -- and members sit in cost-sorted lanes, so a
// group's values are gathered 8-byte loads from a row of npad doubles.  Four steps:
//   hx_sobol_prepare_kernel  lane-local: lane_of_member -> the group-major lane table
//                            tab[k + 2][n_base] (the index loads of the passes are coalesced) and the
//                            groups' use flags; a lane outside 0..npad-1 switches its group off
//   hx_sobol_part_kernel     pass 1, one workgroup per (group chunk, row): a group takes part in a row if it is
//                            in use and none of its k + 2 values is NaN -> on[row][n_base]; the
//                            smallest x_A or x_B of the participants as an integer key and their
//                            count, by integer atomics (as hx_q_minmax_kernel)
//   hx_sobol_kernel<TF>      pass 2, one workgroup per (group chunk, row, factor tile): one lane per group per
//                            batch, the 2 + TF gathered loads of every group of the batch in flight
//                            before the arithmetic; 4 + 4 TF private accumulators, all terms >= 0.
//                            A tile re-reads A and B from the cache; tile 0 writes the four A / B sums
//   hx_mom_reduce_kernel     the chunks' partials in ascending order; hx_sobol_finish_kernel turns
//                            the rows' records into shift and n_part
// No floating atomics: a fixed shuffle tree per wavefront, the four wavefronts added in order, one
// partial per (row, chunk) -- the same bits from call to call for one lane order.
// ===========================================================================
#define HXSB_BLOCK 256
#define HXSB_PER 4                            // groups of a row per lane
#define HXSB_CHUNK (HXSB_BLOCK * HXSB_PER)    // groups of a row per workgroup
// (a row's record HxSobRow: hx_post_abi.h)

// Workgroups whose linear ids agree modulo 8 share an XCD and its L2 (a speed matter only).  A
// chunk's gathers touch cache lines all over its row, so the chunks of one row are given ids that
// agree modulo 8: the row comes into ONE L2 once, not into each of them.  The grid is 8 nchunks
// ceil(nrows / 8) workgroups; -> false for the workgroups past the last row.
#define HXSB_XCDS 8
__device__ __forceinline__ bool hxsb_place(int nchunks, int nrows, int *y, int *chunk) {
  const int id = (int)blockIdx.x, slot = id / HXSB_XCDS;
  *y = (slot / nchunks) * HXSB_XCDS + id % HXSB_XCDS;
  *chunk = slot % nchunks;
  return *y < nrows;
}
__host__ inline unsigned hxsb_grid(int nchunks, int nrows) {
  return (unsigned)(HXSB_XCDS * nchunks * ((nrows + HXSB_XCDS - 1) / HXSB_XCDS));
}

__device__ __forceinline__ double hxsb_unkey(hxq_u64 key) {
  const hxq_u64 b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(256) void hx_sobol_prepare_kernel(const int *__restrict__ lane_of_member, int npad,
                                                               int k, int nb,
                                                               const unsigned char *__restrict__ use,
                                                               int *__restrict__ tab,
                                                               unsigned char *__restrict__ flag) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= nb) return;
  bool ok = use ? use[j] != 0 : true;
  for (int r = 0; r < k + 2; ++r) {
    int lane = lane_of_member[(size_t)j * (size_t)(k + 2) + (size_t)r];
    if (lane < 0 || lane >= npad) { lane = 0; ok = false; }   // (every table entry is a lane that may be read)
    tab[(size_t)r * (size_t)nb + (size_t)j] = lane;
  }
  flag[j] = ok ? 1 : 0;
}

// st[row] must be zero on entry (the min key is kept complemented so that zero is the identity of max)
__global__ __launch_bounds__(HXSB_BLOCK) void hx_sobol_part_kernel(const double *__restrict__ var, int npad,
                                                                   int iy0, const int *__restrict__ tab, int nb,
                                                                   int k, const unsigned char *__restrict__ flag,
                                                                   int nchunks, int nrows, HxSobRow *st,
                                                                   unsigned char *__restrict__ on) {
  int y, chunk;
  if (!hxsb_place(nchunks, nrows, &y, &chunk)) return;   // (the same for the whole workgroup)
  const double *row = var + (size_t)(iy0 + y) * npad;
  const int beg = chunk * HXSB_CHUNK, end = min(beg + HXSB_CHUNK, nb);
  hxq_u64 nkmin = 0, cnt = 0;
  // the lane's HXSB_PER groups side by side, every load unconditional (a group past the end reads the
  // chunk's last group and is left out): A and B, then the factors four at a time -- 4 HXSB_PER
  // gathered loads in flight
  const int i0 = beg + (int)threadIdx.x;
  int j[HXSB_PER];
  double xa[HXSB_PER], xb[HXSB_PER];
  bool ok[HXSB_PER];
#pragma unroll
  for (int b = 0; b < HXSB_PER; ++b) {
    j[b] = min(i0 + b * HXSB_BLOCK, end - 1);
    xa[b] = row[tab[j[b]]];
    xb[b] = row[tab[(size_t)nb + j[b]]];
  }
#pragma unroll
  for (int b = 0; b < HXSB_PER; ++b)
    ok[b] = (i0 + b * HXSB_BLOCK < end) & (flag[j[b]] != 0) & (xa[b] == xa[b]) & (xb[b] == xb[b]);
  for (int r0 = 2; r0 < k + 2; r0 += 4) {
    double v[4 * HXSB_PER];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t base = (size_t)min(r0 + u, k + 1) * (size_t)nb;
#pragma unroll
      for (int b = 0; b < HXSB_PER; ++b) v[u * HXSB_PER + b] = row[tab[base + j[b]]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int b = 0; b < HXSB_PER; ++b) ok[b] = ok[b] & (v[u * HXSB_PER + b] == v[u * HXSB_PER + b]);
  }
#pragma unroll
  for (int b = 0; b < HXSB_PER; ++b) {
    if (i0 + b * HXSB_BLOCK < end) on[(size_t)y * (size_t)nb + j[b]] = ok[b] ? 1 : 0;
    if (ok[b]) {
      nkmin = max(nkmin, max(~hxq_key(xa[b]), ~hxq_key(xb[b])));
      ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nkmin = max(nkmin, __shfl_down(nkmin, off, 64));
    cnt += __shfl_down(cnt, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    HxSobRow *o = st + y;
    atomicMax(&o->nkmin, nkmin); atomicAdd(&o->cnt, cnt);
  }
}

// part[(row * nchunks + chunk) * (4 + 4 k) + ...] = SA1, SA2, SB1, SB2, then T_i, TT_i, F_i, FF_i of
// the chunk; the workgroup (chunk, row, tile) writes the columns of the factors tile * TF ..
template <int TF>
__global__ __launch_bounds__(HXSB_BLOCK) void hx_sobol_kernel(const double *__restrict__ var, int npad, int iy0,
                                                              const int *__restrict__ tab, int nb, int k,
                                                              const HxSobRow *__restrict__ st,
                                                              const unsigned char *__restrict__ on,
                                                              int nchunks, int nrows, double *__restrict__ part) {
  constexpr int NCB = 4 + 4 * TF;
  constexpr int B = TF <= 4 ? HXSB_PER : HXSB_PER / 2;   // groups of a lane in flight at once
  static_assert(HXSB_BLOCK == 256, "the combine below adds four wavefronts in a fixed order");
  __shared__ double red[HXSB_BLOCK / 64][NCB];
  const int tid = (int)threadIdx.x;
  int y, chunk;
  if (!hxsb_place(nchunks, nrows, &y, &chunk)) return;   // (the same for the whole workgroup: no barrier is skipped by a part of it)
  const int f0 = (int)blockIdx.y * TF, nf = min(TF, k - f0);
  const double *row = var + (size_t)(iy0 + y) * npad;
  const unsigned char *onrow = on + (size_t)y * (size_t)nb;
  const int beg = chunk * HXSB_CHUNK, end = min(beg + HXSB_CHUNK, nb);
  const double c = st[y].cnt ? hxsb_unkey(~st[y].nkmin) : 0.0;   // (nobody takes part: no term uses it)
  double acc[NCB];
#pragma unroll
  for (int a = 0; a < NCB; ++a) acc[a] = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < HXSB_PER; j0 += B) {
    const int i0 = beg + j0 * HXSB_BLOCK + tid;
    if (i0 - tid >= end) break;   // (the same for the whole workgroup)
    double xa[B], xb[B], xf[TF * B];
    int la[B], lb[B], lf[TF * B];
    unsigned char o[B];
    bool p[B];
    // every load is unconditional, the table's first, then the gathers: a group past the end reads
    // the chunk's last group and is off, a factor past the tile's last reads that one again (its
    // accumulators are not written)
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int j = min(i0 + b * HXSB_BLOCK, end - 1);
      o[b] = onrow[j];
      la[b] = tab[j];
      lb[b] = tab[(size_t)nb + j];
#pragma unroll
      for (int f = 0; f < TF; ++f) lf[f * B + b] = tab[(size_t)(2 + f0 + min(f, nf - 1)) * (size_t)nb + j];
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      xa[b] = row[la[b]];
      xb[b] = row[lb[b]];
#pragma unroll
      for (int f = 0; f < TF; ++f) xf[f * B + b] = row[lf[f * B + b]];
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      p[b] = (i0 + b * HXSB_BLOCK < end) & (o[b] != 0);
      const double dA = p[b] ? xa[b] - c : 0.0, dB = p[b] ? xb[b] - c : 0.0;
      acc[0] += dA;
      acc[1] += dA * dA;
      acc[2] += dB;
      acc[3] += dB * dB;
#pragma unroll
      for (int f = 0; f < TF; ++f) {
        const double e = p[b] ? xa[b] - xf[f * B + b] : 0.0, g = p[b] ? xb[b] - xf[f * B + b] : 0.0;
        const double t = e * e, u = g * g;
        acc[4 + 4 * f] += t;
        acc[5 + 4 * f] += t * t;
        acc[6 + 4 * f] += u;
        acc[7 + 4 * f] += u * u;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NCB; ++a) {
    double v = acc[a];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6][a] = v;
  }
  __syncthreads();
  if (tid < NCB) {
    const int f = (tid - 4) >> 2;
    const bool mine = tid < 4 ? blockIdx.y == 0 : f < nf;
    const int col = tid < 4 ? tid : 4 + 4 * (f0 + f) + ((tid - 4) & 3);
    if (mine)
      part[((size_t)y * nchunks + chunk) * (size_t)(4 + 4 * k) + col] =
          ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

__global__ __launch_bounds__(256) void hx_sobol_finish_kernel(const HxSobRow *__restrict__ st, int nrows,
                                                              double *__restrict__ shift,
                                                              long long *__restrict__ npart) {
  const int y = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (y >= nrows) return;
  shift[y] = st[y].cnt ? hxsb_unkey(~st[y].nkmin) : __builtin_nan("");
  npart[y] = (long long)st[y].cnt;
}

int hx_sobol_chunks(int nb) { return (nb + HXSB_CHUNK - 1) / HXSB_CHUNK; }
hipError_t hx_launch_sobol_prepare(const int *lane_of_member, int npad, int k, int nb, const unsigned char *use,
                                   int *tab, unsigned char *flag, hipStream_t st) {
  hipLaunchKernelGGL(hx_sobol_prepare_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, lane_of_member, npad, k, nb,
                     use, tab, flag);
  return hipGetLastError();
}
// pass 1.  st: [nrows][2] zeroed; on: [nrows][nb] bytes
hipError_t hx_launch_sobol_part(const double *var, int npad, int iy0, int nrows, const int *tab, int nb, int k,
                                const unsigned char *flag, void *st, unsigned char *on, hipStream_t stream) {
  if (k < 1 || k > HX_SOBOL_MAX_FACTORS || nb < 1 || nrows < 1) return hipErrorInvalidValue;
  const int nchunks = hx_sobol_chunks(nb);
  hipLaunchKernelGGL(hx_sobol_part_kernel, dim3(hxsb_grid(nchunks, nrows)), dim3(HXSB_BLOCK), 0, stream, var, npad,
                     iy0, tab, nb, k, flag, nchunks, nrows, static_cast<HxSobRow *>(st), on);
  return hipGetLastError();
}
// pass 2 over what pass 1 left.  part: [nrows][hx_sobol_chunks(nb)][4 + 4 k] scratch; sums: [nrows][4 + 4 k];
// shift, npart: [nrows]
hipError_t hx_launch_sobol_sums(const double *var, int npad, int iy0, int nrows, const int *tab, int nb, int k,
                                const void *st, const unsigned char *on, double *part, double *sums, double *shift,
                                long long *npart, hipStream_t stream) {
  if (k < 1 || k > HX_SOBOL_MAX_FACTORS || nb < 1 || nrows < 1) return hipErrorInvalidValue;
  const int nchunks = hx_sobol_chunks(nb), nc = 4 + 4 * k;
  const HxSobRow *rec = static_cast<const HxSobRow *>(st);
  if (k <= 4)
    hipLaunchKernelGGL(hx_sobol_kernel<4>, dim3(hxsb_grid(nchunks, nrows), 1), dim3(HXSB_BLOCK), 0, stream, var,
                       npad, iy0, tab, nb, k, rec, on, nchunks, nrows, part);
  else
    hipLaunchKernelGGL(hx_sobol_kernel<8>, dim3(hxsb_grid(nchunks, nrows), (k + 7) / 8), dim3(HXSB_BLOCK), 0, stream,
                       var, npad, iy0, tab, nb, k, rec, on, nchunks, nrows, part);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = nrows * nc;
  hipLaunchKernelGGL(hx_mom_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, part, nchunks, nc, total,
                     sums);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(hx_sobol_finish_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, rec, nrows, shift,
                     npart);
  return hipGetLastError();
}

// ===========================================================================
// Year-by-year co-moments of two windows of rows (hx_ensemble_comoments in hector_amd.h defines the
// sums): cross[a][b] = sum over the members of (q d_a) d_b, a Gram matrix contracted over the member
// axis on the fp64 matrix pipe.  Four steps:
//   hx_mom_prepare_kernel  (npred = 0) the integer weights to lane order, padding lanes 0
//   hx_co_mask_kernel      lane-local: q = 0 where any row of either window is NaN (complete cases)
//   hx_q_minmax_kernel     with that q: every row's smallest participating value, W and the count;
//                          hx_moments_kernel<0> then gives the rows' own sums
//   hx_co_gram_kernel      grid (member chunks, row-tile pairs), 4 wavefronts: a workgroup holds an
//                          HXC_TILE x HXC_TILE block of the matrix, a wavefront 2 x 2 tiles of
//                          16 x 16 in 16 accumulator registers a lane.  v_mfma_f64_16x16x4_f64 takes
//                          A[i][k] from lane (i = lane & 15, k = lane >> 4) and B[k][j] from lane
//                          (j = lane & 15, k = lane >> 4); the four k of one instruction may be ANY
//                          four members, so lane (c, g) owns the HXC_PER consecutive members
//                          m0 + HXC_PER g .. of row a0 + c -- half a cache line, four 16-byte loads
//                          from the row as it sits in memory -- and instruction j contracts the
//                          members m0 + HXC_PER g + j, g < 4.  The weight, the shifts and the
//                          participation select are applied in registers on the way in: no LDS.
// Split-k: a chunk of members per workgroup, one partial block per chunk, and hx_co_reduce_kernel
// adds the chunks in ascending order (no floating atomics: the same bits from call to call).  The
// symmetric call computes the tile pairs on or above the diagonal only and the reduce mirrors the
// entries above the diagonal, so cross is symmetric bit for bit.
// ===========================================================================
#define HXC_TILE 64       // rows of either window per workgroup
#define HXC_CHUNK 1024    // members per workgroup at the least; the host takes a multiple of it
#define HXC_PER 8         // consecutive members of a row per lane and step (16, a full line: measured slower)
#define HXC_STEP (4 * HXC_PER)   // members per wavefront and step
#define HXC_PART_WORDS (8u << 20)   // the host grows the chunk until the partials fit (64 MiB)

// q_lane / qd_lane (lane order, padding lanes 0): zeroed where a value of any of the na rows of A
// or the nb rows of B is NaN; a lane whose q is 0 already reads nothing
__global__ __launch_bounds__(256) void hx_co_mask_kernel(const double *__restrict__ va, int ia0, int na,
                                                         const double *__restrict__ vb, int ib0, int nb,
                                                         int npad, hxq_u64 *__restrict__ q_lane,
                                                         double *__restrict__ qd_lane) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= npad) return;
  if (!q_lane[i]) return;
  bool bad = false;
  const double *pa = va + (size_t)ia0 * npad + i;
#pragma unroll 8
  for (int r = 0; r < na; ++r) { const double x = pa[(size_t)r * npad]; bad = bad || x != x; }
  const double *pb = vb + (size_t)ib0 * npad + i;
#pragma unroll 8
  for (int r = 0; r < nb; ++r) { const double x = pb[(size_t)r * npad]; bad = bad || x != x; }
  if (bad) { q_lane[i] = 0; qd_lane[i] = 0.0; }
}

// part[(chunk * na + a) * nb + b]; mchunk: a multiple of HXC_STEP; mend: the members to go through,
// <= npad and a multiple of HXC_STEP (lanes >= n hold qd = 0)
__global__ __launch_bounds__(256) void hx_co_gram_kernel(const double *__restrict__ va, int ia0, int na,
                                                         const double *__restrict__ vb, int ib0, int nb,
                                                         int npad, int mend, int mchunk, int sym,
                                                         const double *__restrict__ qd,
                                                         const double *__restrict__ shift_a,
                                                         const double *__restrict__ shift_b,
                                                         double *__restrict__ part) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  typedef double d2 __attribute__((ext_vector_type(2)));
  static_assert(HXC_TILE == 64 && HXC_PER % 2 == 0, "four wavefronts of 2 x 2 tiles; 16-byte loads");
  const int nbb = (nb + HXC_TILE - 1) / HXC_TILE;
  const int bi = (int)blockIdx.y / nbb, bj = (int)blockIdx.y - bi * nbb;
  if (sym && bj < bi) return;   // (the whole workgroup: the reduce reads the mirrored entry)
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  // (a diagonal block's lower 32 x 32 quadrant lies below the diagonal: the reduce never reads it)
  if (sym && bj == bi && wave == 2) return;
  const int a0 = bi * HXC_TILE + 32 * (wave >> 1), b0 = bj * HXC_TILE + 32 * (wave & 1);
  // rows past the window are read as its last row (inside the block) and not stored
  const double *ra[2], *rb[2];
  double ca[2], cb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = min(a0 + 16 * t + c, na - 1), b = min(b0 + 16 * t + c, nb - 1);
    ra[t] = va + (size_t)(ia0 + a) * npad + HXC_PER * g;
    rb[t] = vb + (size_t)(ib0 + b) * npad + HXC_PER * g;
    ca[t] = shift_a[a];
    cb[t] = shift_b[b];
  }
  const double *qp = qd + HXC_PER * g;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0, 0, 0, 0};
  const int mbeg = (int)blockIdx.x * mchunk, mstop = min(mbeg + mchunk, mend);
  for (int m = mbeg; m < mstop; m += HXC_STEP) {
    double w[HXC_PER], xa[2][HXC_PER], xb[2][HXC_PER];
#pragma unroll
    for (int j = 0; j < HXC_PER; j += 2) {
      const d2 v = *reinterpret_cast<const d2 *>(qp + m + j);
      w[j] = v.x; w[j + 1] = v.y;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const d2 u = *reinterpret_cast<const d2 *>(ra[t] + m + j);
        const d2 s = *reinterpret_cast<const d2 *>(rb[t] + m + j);
        xa[t][j] = u.x; xa[t][j + 1] = u.y;
        xb[t][j] = s.x; xb[t][j + 1] = s.y;
      }
    }
#pragma unroll
    for (int j = 0; j < HXC_PER; ++j) {
      const bool on = w[j] > 0.0;   // (a participant: none of its values is NaN, the shifts are members' values)
      double A[2], B[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        A[t] = on ? w[j] * (xa[t][j] - ca[t]) : 0.0;
        B[t] = on ? xb[t][j] - cb[t] : 0.0;
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[ti], B[tj], acc[ti][tj], 0, 0, 0);
    }
  }
  // D[(lane >> 4) + 4 r][lane & 15]
  double *po = part + (size_t)blockIdx.x * (size_t)na * (size_t)nb;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = a0 + 16 * ti + g + 4 * r, b = b0 + 16 * tj + c;
        if (a < na && b < nb) po[(size_t)a * nb + b] = acc[ti][tj][r];
      }
}

// cross[a][b] = the chunks' partials added in ascending chunk order; sym: the entry below the
// diagonal is the one above it
__global__ __launch_bounds__(256) void hx_co_reduce_kernel(const double *__restrict__ part, int nchunks, int na,
                                                           int nb, int sym, double *__restrict__ cross) {
  const size_t total = (size_t)na * (size_t)nb;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int a = (int)(idx / (size_t)nb), b = (int)(idx - (size_t)a * nb);
  if (sym && a > b) { const int t = a; a = b; b = t; }
  const double *p = part + (size_t)a * nb + b;
  double s = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) s += p[(size_t)ch * total];
  cross[idx] = s;
}

hipError_t hx_launch_co_mask(const double *va, int ia0, int na, const double *vb, int ib0, int nb, int npad,
                             unsigned long long *q_lane, double *qd_lane, hipStream_t st) {
  hipLaunchKernelGGL(hx_co_mask_kernel, dim3((npad + 255) / 256), dim3(256), 0, st, va, ia0, na, vb, ib0, nb,
                     npad, q_lane, qd_lane);
  return hipGetLastError();
}
// the members a workgroup takes: the smallest multiple of HXC_CHUNK with which the partials of an
// na x nb matrix stay within HXC_PART_WORDS doubles (one chunk, whatever its size, if even two do not)
int hx_co_chunk(int n, int na, int nb) {
  const size_t cell = (size_t)na * (size_t)nb;
  size_t maxchunks = HXC_PART_WORDS / cell;
  if (maxchunks < 1) maxchunks = 1;
  const size_t base = ((size_t)n + HXC_CHUNK - 1) / HXC_CHUNK;   // chunks of HXC_CHUNK
  const size_t k = (base + maxchunks - 1) / maxchunks;
  return (int)((k ? k : 1) * HXC_CHUNK);
}
int hx_co_chunks(int n, int na, int nb) {
  const int ch = hx_co_chunk(n, na, nb);
  return (n + ch - 1) / ch;
}
// part: [hx_co_chunks][na][nb] scratch; cross: [na][nb]; npad must be a multiple of HXC_STEP
hipError_t hx_launch_co_gram(const double *va, int ia0, int na, const double *vb, int ib0, int nb, int n,
                             int npad, int sym, const double *qd, const double *shift_a,
                             const double *shift_b, double *part, double *cross, hipStream_t st) {
  if (npad % HXC_STEP || n > npad || na < 1 || nb < 1) return hipErrorInvalidValue;
  const int chunk = hx_co_chunk(n, na, nb), nchunks = hx_co_chunks(n, na, nb);
  const int mend = (n + HXC_STEP - 1) / HXC_STEP * HXC_STEP;
  const int nba = (na + HXC_TILE - 1) / HXC_TILE, nbb = (nb + HXC_TILE - 1) / HXC_TILE;
  hipLaunchKernelGGL(hx_co_gram_kernel, dim3(nchunks, nba * nbb), dim3(256), 0, st, va, ia0, na, vb, ib0, nb,
                     npad, mend, chunk, sym, qd, shift_a, shift_b, part);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const size_t total = (size_t)na * (size_t)nb;
  hipLaunchKernelGGL(hx_co_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, nchunks,
                     na, nb, sym, cross);
  return hipGetLastError();
}

// ===========================================================================
// Score against observations with correlated errors (hx_member_score_whitened in hector_amd.h defines
// it): chi2[lane] = sum_i y_i^2, Y = W R with W the lower-triangular whitening matrix and R the
// residuals [year k][member], on v_mfma_f64_16x16x4_f64 with M = whitened component i, N = member,
// K = year k.  A[i][k] comes from lane (i = lane & 15, k = lane >> 4), B[k][j] from lane
// (member j = lane & 15, k = lane >> 4), D sits at row (lane >> 4) + 4 reg, column lane & 15.
//   Ownership   one wavefront a workgroup; it owns MT tiles of HXW_TILE members and all NT tiles of
//               HXW_TILE outputs, 4 NT MT <= 64 accumulator doubles a lane for <4,4> (n <= 64), <8,2>
//               (n <= 128), <12,1> (n <= 192: an annual instrumental record) and <16,1> (n <= 256):
//               nothing is exchanged with another wavefront, no partials, no atomics, no LDS.
//   Loop        k0 in steps of 4.  Lane (c, g) reads x[iy[k0 + g]][m0 + 16 t + c] -- four whole
//               128-byte segments of the [year][lane] rows a load, every row read once -- a step
//               ahead of its use, and forms r with two IEEE subtractions.  The row number is read
//               two steps ahead, so no load waits for another.
//   W           the host (EnsembleCore::member_score_whitened) packs it in fragment order,
//               wf[((k0 / 4) NT + tile) 64 + lane], so that an A fragment is one 512-byte read from
//               L2; entries with k > i, i >= n or k >= n are written as exact 0.0 THERE: the caller's
//               upper triangle is never read, let alone multiplied in.  r is selected to an exact 0.0
//               for k >= n.  Output tiles wholly above the diagonal (16 tile + 15 < k0) are skipped:
//               the k loop is unrolled over the tile T the diagonal crosses, and the code of T
//               holds the tiles T .. NT - 1 only, without a branch among its loads and MFMAs.  A
//               tile past n inside the template (zero rows: an exact 0) is computed, which is why
//               there are four sizes and not three.
//   Reduction   a lane squares its 4 values of every tile and adds them in ascending (tile, reg)
//               order, then the four lane groups g are added by xor 16, xor 32 -- (s_g + s_g^1) +
//               (s_g^2 + s_g^3), the same bits in every group since IEEE addition commutes -- and
//               the lanes g = 0 store to the lane-ordered buffer; hx_launch_gather brings it to
//               member order.  Every member's sums are formed in one fixed order, whatever column it
//               sits in; columns >= n members or >= npad are computed from whatever they hold and
//               not stored.
// ===========================================================================
#define HXW_TILE 16       // members per B tile, outputs per A tile (the MFMA's M and N)
#define HXW_ACC 16        // NT x MT at the most: a wavefront takes MT = HXW_ACC / NT tiles of members, 64, 32 or 16 members
#define HXW_MAX 256       // HX_SCORE_WHITENED_MAX
static_assert(HXW_MAX == HX_SCORE_WHITENED_MAX, "the header's limit");

// the template's padded size for n observations: 64, 128, 192 or 256
int hx_sw_padded(int n) { return n <= 64 ? 64 : n <= 128 ? 128 : n <= 192 ? 192 : HXW_MAX; }

// wf[np x np] in fragment order from whiten[n x n] (row-major; only k <= i is read)
void hx_sw_pack(const double *whiten, int n, double *wf) {
  const int np = hx_sw_padded(n), nt = np / HXW_TILE;
  for (int ks = 0; ks < np / 4; ++ks)
    for (int tile = 0; tile < nt; ++tile)
      for (int lane = 0; lane < 64; ++lane) {
        const int i = HXW_TILE * tile + (lane & 15), k = 4 * ks + (lane >> 4);
        wf[((size_t)ks * nt + tile) * 64 + lane] = (i < n && k <= i) ? whiten[(size_t)i * n + k] : 0.0;
      }
}

// iy[np + 8], obs[np + 8] (padded: a valid row, any finite value); base: nullptr = none, else [npad]
template <int NT, int MT>
__global__ __launch_bounds__(64) void hx_score_whiten_kernel(const double *__restrict__ var, int nmem, int npad,
                                                             const int *__restrict__ iy,
                                                             const double *__restrict__ obs,
                                                             const double *__restrict__ wf, int n,
                                                             const double *__restrict__ base,
                                                             double *__restrict__ out) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  static_assert(NT * MT <= HXW_ACC && NT * HXW_TILE <= HXW_MAX, "64 accumulator doubles a lane at the most");
  const int lane = (int)threadIdx.x, c = lane & 15, g = lane >> 4;
  const int m0 = (int)blockIdx.x * (MT * HXW_TILE);
  int col[MT];
  double bs[MT], x[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    col[t] = min(m0 + HXW_TILE * t + c, npad - 1);   // (a column past the block: read inside it, never stored)
    bs[t] = base ? base[col[t]] : 0.0;
  }
  d4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = d4{0, 0, 0, 0};
  const int ntiles = (n + HXW_TILE - 1) / HXW_TILE;
  // lane group g takes year k0 + g of a step: its row number is read two steps ahead of its use,
  // its values and its observation one step ahead (iy and obs are padded by two steps)
  int rnext = iy[4 + g];
  double onext = obs[g];
  {
    const size_t r = (size_t)iy[g] * (size_t)npad;
#pragma unroll
    for (int t = 0; t < MT; ++t) x[t] = var[r + (size_t)col[t]];
  }
  // T: the output tile the diagonal crosses during these four steps; the tiles below T are wholly
  // above the diagonal and do not appear in the code of this T at all
#pragma unroll
  for (int T = 0; T < NT; ++T) {
    if (T < ntiles) {
      const int kend = min(HXW_TILE * (T + 1), n);
      for (int k0 = HXW_TILE * T; k0 < kend; k0 += 4) {
        const double *wk = wf + (size_t)(k0 >> 2) * (NT * 64) + lane;
        double a[NT];
#pragma unroll
        for (int i = T; i < NT; ++i) a[i] = wk[i * 64];   // (a tile past n: packed zeros, an exact 0)
        const double o = onext;
        const bool on = k0 + g < n;
        double r[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const double d = (x[t] - bs[t]) - o;   // (no baseline: bs = 0.0 and x - 0.0 is x, bit for bit)
          r[t] = on ? d : 0.0;
        }
        // the next step's rows, in flight during this step's contraction (past n: the padding's valid row)
        const size_t rn = (size_t)rnext * (size_t)npad;
#pragma unroll
        for (int t = 0; t < MT; ++t) x[t] = var[rn + (size_t)col[t]];
        onext = obs[k0 + 4 + g];
        rnext = iy[k0 + 8 + g];
#pragma unroll
        for (int i = T; i < NT; ++i)
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[i][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], r[t], acc[i][t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) s += acc[i][t][q] * acc[i][t][q];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const int m = m0 + HXW_TILE * t + c;
    if (g == 0 && m < nmem) out[m] = s;
  }
}

// iy / obs: [hx_sw_padded(n) + 8]; wf: hx_sw_pack's; base: nullptr or [npad]; out: [npad] in lane order
hipError_t hx_launch_score_whiten(const double *var, int nmem, int npad, const int *iy, const double *obs,
                                  const double *wf, int n, const double *base, double *out, hipStream_t st) {
  if (n < 1 || n > HXW_MAX || nmem < 1 || nmem > npad) return hipErrorInvalidValue;
#define HXW_CASE(NT, MT) \
  hipLaunchKernelGGL((hx_score_whiten_kernel<NT, MT>), dim3((nmem + MT * HXW_TILE - 1) / (MT * HXW_TILE)), \
                     dim3(64), 0, st, var, nmem, npad, iy, obs, wf, n, base, out)
  if (n <= 64) HXW_CASE(4, 4);
  else if (n <= 128) HXW_CASE(8, 2);
  else if (n <= 192) HXW_CASE(12, 1);
  else HXW_CASE(16, 1);
#undef HXW_CASE
  return hipGetLastError();
}

// ===========================================================================
// Projection of every member's residuals onto a caller's basis (hx_member_project in hector_amd.h
// defines it): Y = B R with B the dense m x n basis and R the residuals [year k][member], on
// v_mfma_f64_16x16x4_f64 with M = output j, N = member, K = year k.  A[j][k] comes from lane
// (j = lane & 15, k = lane >> 4), B[k][member] from lane (member = lane & 15, k = lane >> 4), D sits
// at row (lane >> 4) + 4 reg, column lane & 15 -- the layout of the whitened score above.
//   Ownership   one wavefront a workgroup; it owns HXP_MT tiles of HXP_TILE members (64 members) and
//               all NT = ceil(m / 16) tiles of HXP_TILE outputs, 4 NT HXP_MT <= 64 accumulator doubles
//               a lane: nothing is exchanged with another wavefront, no partials, no atomics, no LDS.
//   Loop        k0 in steps of 4 over all of n (the matrix is dense: no tile is skipped).  Lane (c, g)
//               reads x[iy[k0 + g]][m0 + 16 t + c] -- four whole 128-byte segments of the
//               [year][lane] rows a load, every row read once -- a step ahead of its use, and forms r
//               with two IEEE subtractions.  The row number is read two steps ahead, so no load
//               waits for another; iy and center are padded by two steps with a valid row / 0.0.
//   Basis       the host (EnsembleCore::member_project) packs it in fragment order,
//               bf[((k0 / 4) NT + tile) 64 + lane], so that an A fragment is one 512-byte read from
//               L2; entries with j >= m or k >= n are exact 0.0, and r is selected to an exact 0.0
//               for k >= n.  Every D element is its own chain of fused multiply-adds over k, the
//               same chain in every flavour: an output does not depend on which other rows the
//               basis has, nor on the tile or register its row falls in.
//   Store       lane (c, g), output tile i, member tile t, register q holds output j = 16 i + g + 4 q
//               of member m0 + 16 t + c and writes it to the lane-ordered buffer out[j][npad], sixteen
//               consecutive doubles a lane group, for j < m and member < nmem only; hx_launch_gather
//               with m rows brings it to member order.  Columns >= n members or >= npad are computed
//               from whatever they hold and not stored.
// ===========================================================================
#define HXP_TILE 16          // members per B tile, outputs per A tile (the MFMA's M and N)
#define HXP_MT 4             // member tiles a wavefront: 64 members
#define HXP_MAX_OUT 64       // HX_PROJECT_MAX_OUT: 4 output tiles x HXP_MT = 16 accumulator quads a lane
#define HXP_MAX_YEARS 1024   // HX_PROJECT_MAX_YEARS
static_assert(HXP_MAX_OUT == HX_PROJECT_MAX_OUT && HXP_MAX_YEARS == HX_PROJECT_MAX_YEARS, "the header's limits");
static_assert(HXP_MAX_OUT % HXP_TILE == 0 && HXP_MAX_OUT / HXP_TILE * HXP_MT <= 16, "64 accumulator doubles a lane");

// the steps of 4 years the k loop takes for n years; iy and center hold 4 hx_project_steps(n) + 8 entries
int hx_project_steps(int n) { return (n + 3) / 4; }

// bf[hx_project_steps(n) x NT x 64] in fragment order from basis[m x n] (row-major), NT = ceil(m / 16)
void hx_project_pack(const double *basis, int n, int m, double *bf) {
  const int nt = (m + HXP_TILE - 1) / HXP_TILE, ns = hx_project_steps(n);
  for (int ks = 0; ks < ns; ++ks)
    for (int tile = 0; tile < nt; ++tile)
      for (int lane = 0; lane < 64; ++lane) {
        const int j = HXP_TILE * tile + (lane & 15), k = 4 * ks + (lane >> 4);
        bf[((size_t)ks * nt + tile) * 64 + lane] = (j < m && k < n) ? basis[(size_t)j * n + k] : 0.0;
      }
}

// iy[4 steps + 8], center[4 steps + 8] (padded: a valid row, 0.0); base: nullptr = none, else [npad]
template <int NT>
__global__ __launch_bounds__(64) void hx_project_kernel(const double *__restrict__ var, int nmem, int npad,
                                                        const int *__restrict__ iy,
                                                        const double *__restrict__ center,
                                                        const double *__restrict__ bf, int n, int m,
                                                        const double *__restrict__ base,
                                                        double *__restrict__ out) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  static_assert(NT >= 1 && NT * HXP_TILE <= HXP_MAX_OUT, "64 accumulator doubles a lane at the most");
  const int lane = (int)threadIdx.x, c = lane & 15, g = lane >> 4;
  const int m0 = (int)blockIdx.x * (HXP_MT * HXP_TILE);
  int col[HXP_MT];
  double bs[HXP_MT], x[HXP_MT];
#pragma unroll
  for (int t = 0; t < HXP_MT; ++t) {
    col[t] = min(m0 + HXP_TILE * t + c, npad - 1);   // (a column past the block: read inside it, never stored)
    bs[t] = base ? base[col[t]] : 0.0;
  }
  d4 acc[NT][HXP_MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < HXP_MT; ++t) acc[i][t] = d4{0, 0, 0, 0};
  // lane group g takes year k0 + g of a step: its row number is read two steps ahead of its use,
  // its values and its centre one step ahead (iy and center are padded by two steps)
  int rnext = iy[4 + g];
  double cnext = center[g];
  {
    const size_t r = (size_t)iy[g] * (size_t)npad;
#pragma unroll
    for (int t = 0; t < HXP_MT; ++t) x[t] = var[r + (size_t)col[t]];
  }
  for (int k0 = 0; k0 < n; k0 += 4) {
    const double *bk = bf + (size_t)(k0 >> 2) * (NT * 64) + lane;
    double a[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) a[i] = bk[i * 64];   // (j >= m, k >= n: packed zeros)
    const double o = cnext;
    const bool on = k0 + g < n;
    double r[HXP_MT];
#pragma unroll
    for (int t = 0; t < HXP_MT; ++t) {
      const double d = (x[t] - bs[t]) - o;   // (no baseline: bs = 0.0 and x - 0.0 is x, bit for bit)
      r[t] = on ? d : 0.0;
    }
    // the next step's rows, in flight during this step's contraction (past n: the padding's valid row)
    const size_t rn = (size_t)rnext * (size_t)npad;
#pragma unroll
    for (int t = 0; t < HXP_MT; ++t) x[t] = var[rn + (size_t)col[t]];
    cnext = center[k0 + 4 + g];
    rnext = iy[k0 + 8 + g];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int t = 0; t < HXP_MT; ++t)
        acc[i][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], r[t], acc[i][t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < HXP_MT; ++t) {
    const int mem = m0 + HXP_TILE * t + c;
    if (mem < nmem) {
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = HXP_TILE * i + g + 4 * q;
          if (j < m) out[(size_t)j * (size_t)npad + (size_t)mem] = acc[i][t][q];
        }
    }
  }
}

// iy / center: [4 hx_project_steps(n) + 8]; bf: hx_project_pack's; base: nullptr or [npad]; out: [m][npad] in lane order
hipError_t hx_launch_project(const double *var, int nmem, int npad, const int *iy, const double *center,
                             const double *bf, int n, int m, const double *base, double *out, hipStream_t st) {
  if (n < 1 || n > HXP_MAX_YEARS || m < 1 || m > HXP_MAX_OUT || nmem < 1 || nmem > npad) return hipErrorInvalidValue;
#define HXP_CASE(NT) \
  hipLaunchKernelGGL((hx_project_kernel<NT>), dim3((nmem + HXP_MT * HXP_TILE - 1) / (HXP_MT * HXP_TILE)), \
                     dim3(64), 0, st, var, nmem, npad, iy, center, bf, n, m, base, out)
  const int nt = (m + HXP_TILE - 1) / HXP_TILE;
  if (nt == 1) HXP_CASE(1);
  else if (nt == 2) HXP_CASE(2);
  else if (nt == 3) HXP_CASE(3);
  else HXP_CASE(4);
#undef HXP_CASE
  return hipGetLastError();
}
#endif  // !HX_HOST_EMULATION
