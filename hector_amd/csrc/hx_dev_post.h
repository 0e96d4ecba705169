// hx_dev_post.h -- what a user does with a finished ensemble, on the device: a per-member misfit
// of a recorded output against an observation series (hx_score_kernel) and exact per-year
// weighted quantiles over the members (hx_q_* kernels).  The reference has no counterpart: its
// hosts aggregate fetchvars() data frames in R.  Compiled for the GPU through hx_post.hip -- a
// translation unit of its own, so the year-loop kernels' code generation does not see it -- and
// for the host-emulation build through ensemble_core.cpp (score kernel only: the quantile kernels
// are cooperative -- LDS atomics, cross-lane -- and one lane at a time cannot run them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
#define HXQ_MAXP 16
typedef unsigned long long hxq_u64;

struct HxQYear { hxq_u64 nkmin, kmax, W, cnt; };  // ~(min key), max key, sum of q, members taking part

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
#endif  // !HX_HOST_EMULATION
