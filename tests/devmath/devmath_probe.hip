// TEST INFRASTRUCTURE ONLY: devmath_probe.hip -- the hand-written fp64 device math of the run
// kernels (hx_dev_math.h, hx_dev_chem.h, hx_dev_solver.h), one function at a time.
//
// The product's device headers are included UNCHANGED, in hx_kernels.hip's order, and every group
// of operations gets one small kernel: one thread = one input point.  The constants travel the
// way the run kernels pass them: a kernel-argument struct in device memory that holds an HxConst
// filled by hx_fill_math_table / hx_fill_chem_table / hx_fill_chem_fit, read through a
// `const ProbeArgs *__restrict__` (wide scalar loads; chem_constants_fit keeps its asm form).
//
// Built twice (Makefile): for gfx950 with the product's flags, and for the host through
// tests/emul/shim.  The C entry points take host arrays, own every allocation they touch (hipMalloc,
// copy in, ONE launch, synchronise, copy out, hipFree) and return the first non-zero hipError_t.
// tests/devmath/devmath_checks.py holds them against tests/golden/devmath_reference.npz.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <math.h>
#include <stdint.h>

#include <hx_addrspace.h>

#include "hx_layout.h"

#define HX_DBLK 32
#define HX_KPAD 32
#define HX_WAVES_PER_SIMD(B)

#include "hx_dev_const.h"
#include "hx_dev_clock.h"
#include "hx_dev_math.h"
#include "hx_dev_chem.h"
#include "hx_dev_member.h"
#include "hx_dev_solver.h"

#ifdef HX_HOST_EMULATION
static inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
#define DEVMATH_BACKEND "host-emulation"
#else
#define DEVMATH_BACKEND "hip"
#endif

struct ProbeArgs {
  HxConst kc;
  const double *a, *b;   // inputs, n each (b: second operand or null)
  double *out;           // [column][n]
  int n;
};

// Position j of a batch in thread i takes input (i + 5 j) mod n: the positions of one thread hold
// DIFFERENT points (nothing for the compiler to merge), and every point visits every position.
#define DEVMATH_STRIDE 5
namespace {
__device__ __forceinline__ int probe_index() { return (int)(blockIdx.x * blockDim.x + threadIdx.x); }
__device__ __forceinline__ double probe_in(const double *a, int i, int j, int n) {
  return a[(int)(((long long)i + (long long)DEVMATH_STRIDE * j) % n)];
}
template <int N, bool CHUNKS>
__device__ __forceinline__ void probe_exp_form(const double *a, double *out, int i, int n, int &col,
                                               const double *T) {
  double x[N];
#pragma unroll
  for (int j = 0; j < N; ++j) x[j] = probe_in(a, i, j, n);
  if constexpr (CHUNKS) hx_exp_chunks<N>(x, T);
  else hx_exp_batch<N>(x, T);
#pragma unroll
  for (int j = 0; j < N; ++j) out[(size_t)(col + j) * n + i] = x[j];
  col += N;
}
template <int N>
__device__ __forceinline__ void probe_log_form(const double *a, double *out, int i, int n, int &col,
                                               const double *T) {
  double x[N];
#pragma unroll
  for (int j = 0; j < N; ++j) x[j] = probe_in(a, i, j, n);
  hx_log_batch<N>(x, T);
#pragma unroll
  for (int j = 0; j < N; ++j) out[(size_t)(col + j) * n + i] = x[j];
  col += N;
}
template <int N>
__device__ __forceinline__ void probe_ff_form(const double *a, double *out, int i, int n, int &col) {
  double d[N], ff[N];
#pragma unroll
  for (int j = 0; j < N; ++j) d[j] = probe_in(a, i, j, n);
  hx_frozen_fraction_batch<N>(d, ff);
#pragma unroll
  for (int j = 0; j < N; ++j) out[(size_t)(col + j) * n + i] = ff[j];
  col += N;
}
}  // namespace

// exp: hx_exp_batch<1, 3, 8>, hx_exp_chunks<9, 12, 17> -- 50 columns
#define DEVMATH_EXP_COLS 50
template <bool TAB>
__global__ __launch_bounds__(64) void probe_exp_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  const double *T = TAB ? args->kc.mtab : nullptr;
  int col = 0;
  probe_exp_form<1, false>(args->a, args->out, i, n, col, T);
  probe_exp_form<3, false>(args->a, args->out, i, n, col, T);
  probe_exp_form<8, false>(args->a, args->out, i, n, col, T);
  probe_exp_form<9, true>(args->a, args->out, i, n, col, T);
  probe_exp_form<12, true>(args->a, args->out, i, n, col, T);
  probe_exp_form<17, true>(args->a, args->out, i, n, col, T);
}
__global__ __launch_bounds__(64) void probe_exp1_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  args->out[i] = hx_exp(args->a[i]);
}
// log: hx_log_batch<1, 2, 4> and hx_log -- 8 columns
#define DEVMATH_LOG_COLS 8
template <bool TAB>
__global__ __launch_bounds__(64) void probe_log_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  const double *T = TAB ? args->kc.mtab : nullptr;
  int col = 0;
  probe_log_form<1>(args->a, args->out, i, n, col, T);
  probe_log_form<2>(args->a, args->out, i, n, col, T);
  probe_log_form<4>(args->a, args->out, i, n, col, T);
  args->out[(size_t)col * n + i] = hx_log(args->a[i], T);
}
// hx_log alone (the special values go through here, not through the batches)
template <bool TAB>
__global__ __launch_bounds__(64) void probe_log1_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  args->out[i] = hx_log(args->a[i], TAB ? args->kc.mtab : nullptr);
}
__global__ __launch_bounds__(64) void probe_sqrt_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  args->out[i] = hx_sqrt(args->a[i]);
}
// frozen fraction: hx_frozen_fraction_batch<1, 4> -- 5 columns
#define DEVMATH_FF_COLS 5
__global__ __launch_bounds__(64) void probe_frozen_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  int col = 0;
  probe_ff_form<1>(args->a, args->out, i, n, col);
  probe_ff_form<4>(args->a, args->out, i, n, col);
}
// hx_recip(b), hx_div(a, b), hx_div_cr(a, b, hx_recip(b)), hx_div1(a, b) -- 4 columns
#define DEVMATH_DIV_COLS 4
__global__ __launch_bounds__(64) void probe_div_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  const double a = args->a[i], b = args->b[i];
  const double r = hx_recip(b);
  args->out[i] = r;
  args->out[(size_t)n + i] = hx_div(a, b);
  args->out[(size_t)2 * n + i] = hx_div_cr(a, b, r);
  args->out[(size_t)3 * n + i] = hx_div1(a, b);
}
__global__ __launch_bounds__(64) void probe_pow13_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  args->out[i] = pow_m13(args->a[i]);
}
__global__ __launch_bounds__(64) void probe_pow15_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  args->out[i] = pow_m15(args->a[i]);
}
// the twelve carbonate constants of the two boxes: K0, Kw, 1/Kh, K1, K2, Kb of HL, then of LL
#define DEVMATH_CHEM_COLS 12
__global__ __launch_bounds__(64) void probe_chem_fit_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  double e[12];
  chem_constants_fit(args->a[i], args->b[i], args->kc.kfit, e);
#pragma unroll
  for (int f = 0; f < 12; ++f) args->out[(size_t)f * n + i] = e[f];
}
// ... and the formulas themselves, as the run kernel evaluates them outside the fit's interval
// (hx_kernels.hip, phase A); CTAB: chem_exponents' constants as data (HxConst::ctab) or literals
template <bool CTAB>
__global__ __launch_bounds__(64) void probe_chem_formula_kernel(const ProbeArgs *__restrict__ args) {
  const int i = probe_index(), n = args->n;
  if (i >= n) return;
  const HxConst &kc = args->kc;
  const double TcH = args->a[i], TcL = args->b[i];
  double l2[2] = {TcH + 273.15, TcL + 273.15}, e12[12];
  hx_log_batch<2>(l2, kc.mtab);
  chem_exponents(TcH, l2[0], &e12[0], CTAB ? kc.ctab : nullptr);
  chem_exponents(TcL, l2[1], &e12[6], CTAB ? kc.ctab : nullptr);
  hx_exp_chunks<12>(e12, kc.mtab);
#pragma unroll
  for (int f = 0; f < 12; ++f) args->out[(size_t)f * n + i] = e12[f];
}

// ---- host side ------------------------------------------------------------------------------
namespace {
template <class K>
int probe_run(K kernel, const double *a, const double *b, int n, int ncol, double *out) {
  if (n <= 0 || ncol <= 0 || !a || !out) return (int)hipErrorInvalidValue;
  ProbeArgs h{};
  hx_fill_math_table(h.kc.mtab);
  hx_fill_chem_table(h.kc.ctab);
  hx_fill_chem_fit(h.kc.kfit);
  h.n = n;
  double *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
  ProbeArgs *d_args = nullptr;
  const size_t nin = (size_t)n * sizeof(double), nout = (size_t)n * ncol * sizeof(double);
  int rc = 0;
  auto ok = [&rc](hipError_t e) { if (rc == 0 && e != hipSuccess) rc = (int)e; return rc == 0; };
  if (ok(hipMalloc(&d_a, nin)) && (!b || ok(hipMalloc(&d_b, nin))) && ok(hipMalloc(&d_out, nout)) &&
      ok(hipMalloc(&d_args, sizeof(ProbeArgs))) && ok(hipMemcpy(d_a, a, nin, hipMemcpyHostToDevice)) &&
      (!b || ok(hipMemcpy(d_b, b, nin, hipMemcpyHostToDevice)))) {
    h.a = d_a; h.b = d_b; h.out = d_out;
    if (ok(hipMemcpy(d_args, &h, sizeof(ProbeArgs), hipMemcpyHostToDevice))) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)0,
                         (const ProbeArgs *)d_args);
      ok(hipGetLastError());
      ok(hipDeviceSynchronize());
      if (rc == 0) ok(hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost));
    }
  }
  if (d_args) ok(hipFree(d_args));
  if (d_out) ok(hipFree(d_out));
  if (d_b) ok(hipFree(d_b));
  if (d_a) ok(hipFree(d_a));
  return rc;
}
}  // namespace

extern "C" {
const char *devmath_backend() { return DEVMATH_BACKEND; }
int devmath_stride() { return DEVMATH_STRIDE; }
// out: [50][n]
int devmath_exp(const double *x, int n, int table, double *out) {
  return table ? probe_run(probe_exp_kernel<true>, x, nullptr, n, DEVMATH_EXP_COLS, out)
               : probe_run(probe_exp_kernel<false>, x, nullptr, n, DEVMATH_EXP_COLS, out);
}
int devmath_exp1(const double *x, int n, double *out) { return probe_run(probe_exp1_kernel, x, nullptr, n, 1, out); }
// out: [8][n]
int devmath_log(const double *x, int n, int table, double *out) {
  return table ? probe_run(probe_log_kernel<true>, x, nullptr, n, DEVMATH_LOG_COLS, out)
               : probe_run(probe_log_kernel<false>, x, nullptr, n, DEVMATH_LOG_COLS, out);
}
int devmath_log1(const double *x, int n, int table, double *out) {
  return table ? probe_run(probe_log1_kernel<true>, x, nullptr, n, 1, out)
               : probe_run(probe_log1_kernel<false>, x, nullptr, n, 1, out);
}
int devmath_sqrt(const double *x, int n, double *out) { return probe_run(probe_sqrt_kernel, x, nullptr, n, 1, out); }
// out: [5][n]
int devmath_frozen(const double *d, int n, double *out) {
  return probe_run(probe_frozen_kernel, d, nullptr, n, DEVMATH_FF_COLS, out);
}
// out: [4][n]
int devmath_div(const double *a, const double *b, int n, double *out) {
  if (!b) return (int)hipErrorInvalidValue;
  return probe_run(probe_div_kernel, a, b, n, DEVMATH_DIV_COLS, out);
}
int devmath_pow13(const double *x, int n, double *out) { return probe_run(probe_pow13_kernel, x, nullptr, n, 1, out); }
int devmath_pow15(const double *x, int n, double *out) { return probe_run(probe_pow15_kernel, x, nullptr, n, 1, out); }
// out: [12][n]
int devmath_chem_fit(const double *TcH, const double *TcL, int n, double *out) {
  if (!TcL) return (int)hipErrorInvalidValue;
  return probe_run(probe_chem_fit_kernel, TcH, TcL, n, DEVMATH_CHEM_COLS, out);
}
int devmath_chem_formula(const double *TcH, const double *TcL, int n, int table, double *out) {
  if (!TcL) return (int)hipErrorInvalidValue;
  return table ? probe_run(probe_chem_formula_kernel<true>, TcH, TcL, n, DEVMATH_CHEM_COLS, out)
               : probe_run(probe_chem_formula_kernel<false>, TcH, TcL, n, DEVMATH_CHEM_COLS, out);
}
}
