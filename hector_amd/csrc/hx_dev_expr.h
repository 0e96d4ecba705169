// hx_dev_expr.h -- a series from a whole expression in one launch (hx_series_eval in hector_amd.h
// defines every instruction; contraction is off as in the score kernel).  Included from
// hx_dev_post.h, and with it compiled for the GPU through hx_post.hip and for the host-emulation
// build through ensemble_post.cpp: the kernel is lane-local and uses nothing the shim lacks.
//
// One lane per member, grid (lanes / 256, years / R): a lane takes R rows of every DISTINCT operand
// into registers, all loads in flight, and its member values, then walks the postfix program ONCE
// over the batch -- an instruction is fetched through scalar loads from the record (wave-uniform),
// decoded once, and applied to the R rows.  Nothing is indexed at run time in private memory:
//   - the operand batch xv (NV slots of R rows), the member values xm[NV] and the evaluation stack
//     live in registers, addressed by compile-time indices only (a member value is picked by
//     hxe_member, the same chain of compares on the instruction's arg);
//   - the top of the stack is t (R rows); the values below it are the NS - 1 slots of st.  The host writes the
//     stack depth BEFORE each instruction into it (the depth of a postfix program is static), so
//     "the value under the top" is st[depth - 2], picked by a wave-uniform chain of compares over
//     the NS - 1 slots (hxe_get / hxe_put) -- registers selected by the statically known depth;
//   - a push spills t to st[depth - 1] and loads t; a unary works on t; a binary reads one slot, a
//     WHERE two.
// Three instantiations, chosen by the launcher from the operand count and the depth the host found,
// so that a small expression keeps many rows in flight and a large one still fits its registers:
//   <2, 3, 8>   up to 2 operands / 2 member vectors, depth 3: 8 rows a lane
//   <4, 5, 4>   up to 4, depth 5: 4 rows
//   <8, 8, 4>   the limits of hx_series_eval
// Rows behind y_hi are stored as NaN without loads; a batch wholly behind it runs no program.
#pragma once

static_assert(HXE_MAX_INS == HX_EX_MAX_INS && HXE_MAX_TAB == HX_EX_MAX_VARS && HXE_MAX_TAB == HX_EX_MAX_MEMBERS &&
              HXE_MAX_TAB == HX_EX_MAX_YEARVECS, "HxExprProg is sized by the limits of hx_series_eval");

// A batch of R rows is ONE value of a vector type, and the slots are the fields of a struct, not the
// elements of an array: a slot is read or written whole under a chain of compares of the
// wave-uniform idx, written by recursion over the fields.  (Slots in an array end up in private
// memory: a loop over them is folded into one access at a run-time index, and so are the stores of a
// chain of branches, which the compiler merges behind a selected element address.  A field has no
// run-time index to select.)
template <int R> struct HxeRows { typedef double type __attribute__((vector_size(R * sizeof(double)))); };
template <int N, class V> struct HxeSlots { V head; HxeSlots<N - 1, V> tail; };
template <class V> struct HxeSlots<0, V> {};

template <int J, int N, class V>   // slot J, a compile-time index
__device__ __forceinline__ V &hxe_at(HxeSlots<N, V> &s) {
  if constexpr (J == 0) return s.head;
  else return hxe_at<J - 1, N - 1, V>(s.tail);
}
template <int N, class V>
__device__ __forceinline__ void hxe_get(const HxeSlots<N, V> &s, int idx, V &y) {
  if constexpr (N > 0) {
    if (idx == 0) y = s.head;
    else hxe_get<N - 1, V>(s.tail, idx - 1, y);
  }
}
template <int N, class V>
__device__ __forceinline__ void hxe_put(HxeSlots<N, V> &s, int idx, const V &t) {
  if constexpr (N > 0) {
    if (idx == 0) s.head = t;
    else hxe_put<N - 1, V>(s.tail, idx - 1, t);
  }
}
template <int N, class V>
__device__ __forceinline__ void hxe_fill(HxeSlots<N, V> &s, const V &t) {
  if constexpr (N > 0) { s.head = t; hxe_fill<N - 1, V>(s.tail, t); }
}
// rows y0 .. y0 + R - 1 of operand K and of those after it; a row before startDate, behind y_hi, or of
// an operand the program does not have is NaN and not loaded (all wave-uniform)
template <int K, int NV, int R, class V>
__device__ __forceinline__ void hxe_load(HxeSlots<NV, V> &xv, const HxExprProg *__restrict__ P, int nvar, int y0,
                                         int y_hi, int npad, int lane) {
  if constexpr (K < NV) {
    const double *blk = P->var[K];
    const int lag = P->lag[K];
    V x;
#pragma unroll
    for (int e = 0; e < R; ++e) {
      const int y = y0 + e - lag;
      x[e] = __builtin_nan("");
      if (K < nvar && y0 + e <= y_hi && y >= 0) x[e] = blk[(size_t)y * (size_t)npad + (size_t)lane];
    }
    hxe_at<K, NV, V>(xv) = x;
    hxe_load<K + 1, NV, R, V>(xv, P, nvar, y0, y_hi, npad, lane);
  }
}
template <int J, int N>
__device__ __forceinline__ double hxe_member(const double (&xm)[N], int idx) {
  if constexpr (J < N) return idx == J ? xm[J] : hxe_member<J + 1, N>(xm, idx);
  else return 0.0;
}

#ifndef HXE_SMALL_ROWS
#define HXE_SMALL_ROWS 8   // rows a lane of the smallest flavour (an experiment build may set 4 or 16)
#endif
#define HXE_ROWS(expr)                  \
  _Pragma("unroll") for (int e = 0; e < R; ++e) { const double a = y[e], b = t[e]; (void)a; t[e] = (expr); }

template <int NV, int NS, int R>
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
__global__ __launch_bounds__(256) void hx_series_expr_kernel(const HxExprProg *__restrict__ P, int npad, int ns,
                                                             int year_start, int y_hi, double *__restrict__ z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (lane >= npad) return;
  const int y0 = (int)blockIdx.y * R;
  const double nan = __builtin_nan("");
  if (y0 > y_hi) {   // wave-uniform: nothing to load, nothing to evaluate
#pragma unroll
    for (int e = 0; e < R; ++e)
      if (y0 + e < ns) z[(size_t)(y0 + e) * (size_t)npad + (size_t)lane] = nan;
    return;
  }
  const int nvar = P->nvar, nmem = P->nmem, nins = P->nins;
  typedef typename HxeRows<R>::type V;
  HxeSlots<NV, V> xv;
  hxe_load<0, NV, R, V>(xv, P, nvar, y0, y_hi, npad, lane);
  double xm[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) xm[k] = k < nmem ? P->mem[k][lane] : 0.0;
  V t;
#pragma unroll
  for (int e = 0; e < R; ++e) t[e] = 0.0;
  HxeSlots<NS - 1, V> st;
  hxe_fill<NS - 1, V>(st, t);
  for (int i = 0; i < nins; ++i) {
    const unsigned w = P->ins[i];
    const int op = (int)(w & 255u), arg = (int)((w >> 8) & 255u), d = (int)((w >> 16) & 255u);
    if (op <= HX_EX_YEAR) {   // a push: the top goes under, the new value on top
      hxe_put<NS - 1, V>(st, d - 1, t);
      if (op == HX_EX_VAR) {
        hxe_get<NV, V>(xv, arg, t);
      } else if (op == HX_EX_MEMBER) {
        const double v = hxe_member<0, NV>(xm, arg);
#pragma unroll
        for (int e = 0; e < R; ++e) t[e] = v;
      } else if (op == HX_EX_YEARVEC) {
        const double *vec = P->vec[arg];
#pragma unroll
        for (int e = 0; e < R; ++e) t[e] = vec[y0 + e < ns ? y0 + e : ns - 1];
      } else if (op == HX_EX_CONST) {
        const double v = P->cval[i];
#pragma unroll
        for (int e = 0; e < R; ++e) t[e] = v;
      } else {
#pragma unroll
        for (int e = 0; e < R; ++e) t[e] = (double)(year_start + y0 + e);
      }
    } else if (op <= HX_EX_EXP) {   // unary, on the top
      const V &y = t;
      switch (op) {
        case HX_EX_NEG: HXE_ROWS(-b) break;
        case HX_EX_ABS: HXE_ROWS(fabs(b)) break;
        case HX_EX_SQRT: HXE_ROWS(sqrt(b)) break;
        case HX_EX_LOG: HXE_ROWS(log(b)) break;
        default: HXE_ROWS(exp(b)) break;
      }
    } else if (op == HX_EX_WHERE) {   // c a b
      V c = t, y = t;   // (batches of this instruction alone: nothing of them lives across the loop)
      hxe_get<NS - 1, V>(st, d - 3, c);
      hxe_get<NS - 1, V>(st, d - 2, y);
#pragma unroll
      for (int e = 0; e < R; ++e) t[e] = c[e] != c[e] ? nan : (c[e] != 0.0 ? y[e] : t[e]);
    } else {   // binary: a under the top, b the top
      V y = t;
      hxe_get<NS - 1, V>(st, d - 2, y);
      switch (op) {
        case HX_EX_ADD: HXE_ROWS(a + b) break;
        case HX_EX_SUB: HXE_ROWS(a - b) break;
        case HX_EX_MUL: HXE_ROWS(a * b) break;
        case HX_EX_DIV: HXE_ROWS(a / b) break;
        case HX_EX_MIN: HXE_ROWS((a < b || a != a) ? a : b) break;
        case HX_EX_MAX: HXE_ROWS((a > b || a != a) ? a : b) break;
        case HX_EX_LT: HXE_ROWS((a != a || b != b) ? nan : (a < b ? 1.0 : 0.0)) break;
        case HX_EX_LE: HXE_ROWS((a != a || b != b) ? nan : (a <= b ? 1.0 : 0.0)) break;
        case HX_EX_GT: HXE_ROWS((a != a || b != b) ? nan : (a > b ? 1.0 : 0.0)) break;
        case HX_EX_GE: HXE_ROWS((a != a || b != b) ? nan : (a >= b ? 1.0 : 0.0)) break;
        case HX_EX_EQ: HXE_ROWS((a != a || b != b) ? nan : (a == b ? 1.0 : 0.0)) break;
        case HX_EX_NE: HXE_ROWS((a != a || b != b) ? nan : (a != b ? 1.0 : 0.0)) break;
        default: HXE_ROWS(a != a ? b : a) break;   // HX_EX_IFNAN
      }
    }
  }
#pragma unroll
  for (int e = 0; e < R; ++e) {
    const int yy = y0 + e;
    if (yy < ns) z[(size_t)yy * (size_t)npad + (size_t)lane] = yy <= y_hi ? t[e] : nan;
  }
}
#undef HXE_ROWS

// nvar, nmem, depth: what the program uses (the host found them when it translated it): they pick
// the instantiation
hipError_t hx_launch_series_expr(const HxExprProg *prog, int nvar, int nmem, int depth, int npad, int ns,
                                 int year_start, int y_hi, double *z, hipStream_t st) {
  if (nvar < 1 || nvar > HXE_MAX_TAB || nmem < 0 || nmem > HXE_MAX_TAB || depth < 1 || depth > HX_EX_MAX_STACK)
    return hipErrorInvalidValue;
  const dim3 block(256);
#define HXE_LAUNCH(NV, NS, R)                                                                         \
  hipLaunchKernelGGL((hx_series_expr_kernel<NV, NS, R>), dim3((npad + 255) / 256, (ns + R - 1) / R), block, 0, \
                     st, prog, npad, ns, year_start, y_hi, z)
  if (nvar <= 2 && nmem <= 2 && depth <= 3) HXE_LAUNCH(2, 3, HXE_SMALL_ROWS);
  else if (nvar <= 4 && nmem <= 4 && depth <= 5) HXE_LAUNCH(4, 5, 4);
  else HXE_LAUNCH(8, 8, 4);
#undef HXE_LAUNCH
  return hipGetLastError();
}
