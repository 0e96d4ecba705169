// hx_post_abi.h -- what the host runtime and the device code share: the records the host fills or
// reads back, the constants it sizes its buffers by, and the prototypes of every launcher and helper
// the host files call.  Plain C++: no kernels, no device code.  hx_dev_post.h includes it, so its
// launchers are defined against these prototypes and its kernels read the records through the very
// definitions the host wrote them with.  (hx_kernels.hip does not yet: its text keys the committed
// counter profiles, profiles/pmc_index.json; a prototype that drifts from it fails at link time.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct HxArgs;       // hx_layout.h
struct HxDiagArgs;

// ---- records and constants of the post-processing kernels (hx_dev_post.h) -------------------------
// metrics: EnsembleCore::metric_block fills the groups and their row lists
#define HXM_GROUP 4
#define HXM_BATCH 16
#define HXM_PAD 0x40000000   // a list is padded to a multiple of HXM_BATCH with (last row | HXM_PAD): loaded, never consumed
struct HxMetSpec { int op, iy0, iy1, base; double thr, mid; };   // base: which of the group's reference periods, -1 none
struct HxMetGroup {
  int nspec, nbase, brow0, nbrow, wrow0, nwrow, pad0, pad1;   // rows[brow0 .. brow0 + nbrow), rows[wrow0 .. wrow0 + nwrow)
  int b0[HXM_GROUP], b1[HXM_GROUP];
  HxMetSpec s[HXM_GROUP];
};
// pair metrics: EnsembleCore::pair_metric_block
struct HxPairSpec { int op, iy0, iy1, a0, a1, b0, b1, pad; double thr; };   // rows; a0 > a1 / b0 > b1: no reference period
// series: ops of hx_launch_series_ew beside the public HX_SER_*
#define HXS_ANOM_APPLY 100   // internal: z = a - base[lane]
#define HXS_COMBINE 101      // internal: z = (c0 * a) + (c1 * b), the whole-surface combinations
// series from an expression (hx_series_eval): EnsembleCore::series_eval fills the record, the kernel of
// hx_dev_expr.h reads it through scalar loads.  The tables are sized by the limits of hx_series_eval.
#define HXE_MAX_INS 64
#define HXE_MAX_TAB 8
struct HxExprProg {
  const double *var[HXE_MAX_TAB];   // the block of distinct operand k, rows of the current lane order
  const double *mem[HXE_MAX_TAB];   // [npad] a member vector in lane order
  const double *vec[HXE_MAX_TAB];   // [ns] a year vector, NaN outside its span
  double cval[HXE_MAX_INS];         // CONST: the value of instruction i
  unsigned ins[HXE_MAX_INS];        // op | arg << 8 | (stack depth before the instruction) << 16
  int lag[HXE_MAX_TAB];             // operand k is read lag[k] rows earlier
  int nins, nvar, nmem, pad;
};
// quantiles, moments, co-moments: the host (ensemble_post.cpp, hx_fleet.cpp) reads a row's record back
// as four 8-byte words, Sobol's as two, a rank record as four
#define HXQ_MAXP 16
typedef unsigned long long hxq_u64;
struct HxQYear { hxq_u64 nkmin, kmax, W, cnt; };  // ~(min key), max key, sum of q, members taking part
struct HxSobRow { hxq_u64 nkmin, cnt; };          // ~(min key of x_A, x_B), groups taking part
struct HxRankOut { double crps, pit; long long npart, pad; };
static_assert(sizeof(HxQYear) == 4 * 8, "the host indexes HxQYear as st[4 * row + field]");
static_assert(sizeof(HxSobRow) == 2 * 8, "the host sizes SobBuf::st as [rows][2] words");
static_assert(sizeof(HxRankOut) == 4 * 8, "the host indexes HxRankOut as rec[4 * row + field]");

// ---- launchers and helpers defined in hx_kernels.hip ----------------------------------------------
hipError_t hx_launch_spinup(int B, const HxArgs *d_args, int nmem_launch, int *d_steps,
                            hipStream_t st);
int hx_track_value_rows(int B);
int hx_pair_available();
hipError_t hx_launch_run_pair(const HxArgs *d_args, int npad, bool heatflux, bool kpm, int iy_from,
                              int iy_to, hipStream_t st, bool cons, int nbiome);
hipError_t hx_launch_prewarm(const int *d_stop, long long max_ticks, double *d_sink, int waves,
                             const double *mem, unsigned long long n_mem, hipStream_t st);
hipError_t hx_launch_run(int B, const HxArgs *d_args, int npad, bool heatflux, bool kpm, int con,
                         int iy_from, int iy_to, hipStream_t st, bool two_wave, int cus,
                         bool partials = false);
int hx_doeclim_block_years();
int hx_doeclim_kernel_pad();
void hx_fill_chem_table_host(double *t);
hipError_t hx_launch_broadcast(double *table, int nrows, int npad, hipStream_t st);
hipError_t hx_launch_broadcast_u32(unsigned *v, int npad, hipStream_t st);
hipError_t hx_launch_alk(const HxArgs *d_args, int nmem_launch, hipStream_t st);
hipError_t hx_launch_or_flags(unsigned *status, const double *flag_row, int npad, hipStream_t st);
hipError_t hx_launch_gas(const double *par, const double *ser, const double *h0, int nh, int ns,
                         int npad, double *n2o_out, double *rf_other_out, hipStream_t st);
hipError_t hx_launch_diag(int kind, const HxDiagArgs &a, double *out, hipStream_t st);
hipError_t hx_launch_slr(const double *tgav, int npad, int start_year, int iy_to, double *out,
                         size_t var_stride, hipStream_t st);
hipError_t hx_launch_gather(const double *src, const int *lane_of_member, double *dst, int n,
                            int npad, int nyears, hipStream_t st);
hipError_t hx_launch_stats(const double *var, int n, int npad, int iy0, int nyears,
                           double *stats, hipStream_t st);
hipError_t hx_launch_combine_stats(const double *slots, int world, int rows, double *out,
                                   hipStream_t st);
// {n, sum, sum of squares, min, max} of rows iy0 .. iy0 + nyears - 1 from the run kernel's
// per-wavefront partials (HxBuffers::wpart), for one or two of its variables in one launch:
// var[k] 0 = CO2_concentration, 1 = global_tas; rows[k] the variable's output block (the members of
// the first `skip` wavefronts, which wrote no partials, are read from it); out[k] [nyears][5]
hipError_t hx_launch_combine_partials(const double *wpart, int nvar, const int *var,
                                      const double *const *rows, double *const *out, int n, int npad,
                                      int ns, int iy0, int nyears, int skip, hipStream_t st);
// can hx_launch_run(B, .., heatflux, kpm, con, .., two_wave, .., partials = true) be asked for them?
// (hx_run_kernel_stats: the plain one-biome kernel's flavour with the epilogue)
bool hx_run_writes_partials(int B, bool heatflux, bool kpm, int con, bool two_wave);
hipError_t hx_launch_derive(const double *params, double *derived, const double *ker,
                            int ker_per_member, int ns, int nbiome, int npad, hipStream_t st);
hipError_t hx_launch_doeclim_kernel(const double *diff_row, double *ker, int ns, int count,
                                    int stride, hipStream_t st);
hipError_t hx_launch_unit_csys(int n, const double *Tc, const double *carbon, const double *alk,
                               double inv_volume, double *out, hipStream_t st);

// ---- launchers and helpers defined in hx_dev_post.h -----------------------------------------------
// Compiled into hx_post.hip's object for the GPU.  The host-emulation build has the lane-local ones
// (score, metrics, pair metrics, series, mixes) through ensemble_post.cpp and none of the rest: their
// kernels are cooperative, and the verbs that would call them refuse.
hipError_t hx_launch_score(const double *var, int n, int npad, const int *iy, const double *obs,
                           const double *sigma, int nobs, int b0, int b1, double *out, hipStream_t st);
hipError_t hx_launch_metric(const double *var, int n, int npad, const void *groups, int ngroups,
                            const int *rows, int year_start, double *out, hipStream_t st);
hipError_t hx_launch_pair_metric(const double *a, const double *b, const double *bvec, int bvec_iy0, int n,
                                 int npad, const void *specs, int nspecs, double *out, hipStream_t st);
hipError_t hx_launch_series_ew(int op, const double *a, const double *b, const double *bvec, const double *base,
                               int npad, int ns, int y_lo, int y_hi, double c0, double c1, double *z,
                               hipStream_t st);
hipError_t hx_launch_series_base(const double *a, int npad, int r0, int r1, double *base, hipStream_t st);
hipError_t hx_launch_series_cumsum(const double *a, int npad, int ns, int y0, int y_hi, double *z,
                                   hipStream_t st);
hipError_t hx_launch_series_runmean(const double *a, int npad, int ns, int w, int back, int y_hi, double *z,
                                    hipStream_t st);
hipError_t hx_launch_series_permute(const double *src, const int *src_lane, int npad, int ns, double *dst,
                                    hipStream_t st);
hipError_t hx_launch_series_expr(const HxExprProg *prog, int nvar, int nmem, int depth, int npad, int ns,
                                 int year_start, int y_hi, double *z, hipStream_t st);
hipError_t hx_launch_mseries_fill(const double *row, int ns, int npad, double *table, hipStream_t st);
hipError_t hx_launch_mseries_mix(const double *coeff, const int *member_of_lane, int n, int npad, const int *rows,
                                 const double *basis, int nrows, int nbasis, double *table, hipStream_t st);
hipError_t hx_launch_gas_mix(const double *par, const double *ser, const double *h0, const double *nat,
                             const double *molar, const int *rec, const double *coeff, const long long *coff,
                             const double *basis, const int *cover, const int *member_of_lane, int n, int nh,
                             int ns, int npad, double *n2o_out, double *rf_other_out, hipStream_t st);
hipError_t hx_launch_slcf_mix(const double *ser, const double *kon, const int *rec, const double *coeff,
                              const long long *coff, const double *basis, const int *cover,
                              const int *member_of_lane, int n, int ns, int npad, double *const *rows7,
                              const double *const *rho4, hipStream_t st);
hipError_t hx_launch_bin(const double *var, int n, int npad, int iy0, int nrows, const unsigned long long *q,
                         const double *edges, int K, unsigned long long *sums, hipStream_t stream);
hipError_t hx_launch_q_minmax(const double *var, int n, int npad, int iy0, int ny,
                              const unsigned long long *q, void *st, hipStream_t stream);
hipError_t hx_launch_q_init(const void *st, int ny, const double *probs, int np, int skip, int *lo,
                            unsigned long long *prefix, unsigned long long *rem, hipStream_t stream);
hipError_t hx_launch_q_hist(const double *var, int n, int npad, int iy0, int ny,
                            const unsigned long long *q, const int *lo, const unsigned long long *prefix,
                            int np, int aggregate, unsigned long long *hist, hipStream_t stream);
hipError_t hx_launch_q_pick(int ny, int *lo, unsigned long long *prefix, unsigned long long *rem, int np,
                            unsigned long long *hist, hipStream_t stream);
hipError_t hx_launch_mom_prepare(const unsigned long long *q_mem, const double *pred_mem, int npred, int n,
                                 int npad, const int *lane_of_member, const double *c,
                                 unsigned long long *q_lane, double *qd_lane, double *e_lane, hipStream_t st);
int hx_mom_chunks(int n);
hipError_t hx_launch_moments(const double *var, int n, int npad, int iy0, int nrows, const double *qd,
                             const double *e, int npred, const double *shift, double *part, double *out,
                             hipStream_t st);
hipError_t hx_launch_grp_prepare(const int *lab_mem, int n, int npad, const int *lane_of_member, int *lab_lane,
                                 hipStream_t st);
hipError_t hx_launch_gmom_prepare(const unsigned long long *q_mem, const double *pred_mem, const int *lab_mem,
                                  int npred, int n, int npad, const int *lane_of_member, const double *c,
                                  unsigned long long *q_lane, double *qd_lane, double *e_lane, int *lab_lane,
                                  hipStream_t st);
hipError_t hx_launch_gq_minmax(const double *var, int n, int npad, int iy0, int ny, const unsigned long long *q,
                               const int *lab, int G, void *st, hipStream_t stream);
hipError_t hx_launch_gq_hist(const double *var, int n, int npad, int iy0, int ny, const unsigned long long *q,
                             const int *lab, int G, const int *lo, const unsigned long long *prefix, int np,
                             unsigned long long *hist, hipStream_t stream);
hipError_t hx_launch_gbin(const double *var, int n, int npad, int iy0, int nrows, const unsigned long long *q,
                          const int *lab, int G, const double *edges, int K, unsigned long long *sums,
                          hipStream_t stream);
hipError_t hx_launch_gmoments(const double *var, int n, int npad, int iy0, int nrows, const double *qd,
                              const double *e, const int *lab, int G, int npred, const double *shift,
                              double *part, double *out, hipStream_t st);
int hx_sobol_chunks(int nb);
hipError_t hx_launch_sobol_prepare(const int *lane_of_member, int npad, int k, int nb, const unsigned char *use,
                                   int *tab, unsigned char *flag, hipStream_t st);
hipError_t hx_launch_sobol_part(const double *var, int npad, int iy0, int nrows, const int *tab, int nb, int k,
                                const unsigned char *flag, void *st, unsigned char *on, hipStream_t stream);
hipError_t hx_launch_sobol_sums(const double *var, int npad, int iy0, int nrows, const int *tab, int nb, int k,
                                const void *st, const unsigned char *on, double *part, double *sums, double *shift,
                                long long *npart, hipStream_t stream);
hipError_t hx_launch_co_mask(const double *va, int ia0, int na, const double *vb, int ib0, int nb, int npad,
                             unsigned long long *q_lane, double *qd_lane, hipStream_t st);
int hx_co_chunks(int n, int na, int nb);
hipError_t hx_launch_co_gram(const double *va, int ia0, int na, const double *vb, int ib0, int nb, int n,
                             int npad, int sym, const double *qd, const double *shift_a,
                             const double *shift_b, double *part, double *cross, hipStream_t st);
size_t hx_rank_row_words(int n);
size_t hx_rank_scratch_bytes();
hipError_t hx_launch_rank(const double *src, int n, int npad, int row0, const int *rows, int nrows,
                          const unsigned long long *q, int mode, const double *obs, unsigned long long *scratch,
                          double *dst, int dst_row0, void *res, hipStream_t stream);
int hx_sw_padded(int n);
void hx_sw_pack(const double *whiten, int n, double *wf);
hipError_t hx_launch_score_whiten(const double *var, int nmem, int npad, const int *iy, const double *obs,
                                  const double *wf, int n, const double *base, double *out, hipStream_t st);
int hx_project_steps(int n);
void hx_project_pack(const double *basis, int n, int m, double *bf);
hipError_t hx_launch_project(const double *var, int nmem, int npad, const int *iy, const double *center,
                             const double *bf, int n, int m, const double *base, double *out, hipStream_t st);

// ---- the select state of hx_ensemble_quantiles on the host (ensemble_post.cpp; hx_fleet.cpp) -------
namespace hx {
// the same arithmetic as the device's hx_q_init_kernel / hx_q_pick_kernel: st[4] = one HxQYear
int hxq_host_start(const unsigned long long *st, unsigned long long *pre);
unsigned long long hxq_host_target(double p, unsigned long long W);
// one probability of one year: hist[256] -> prefix and remaining rank updated for the digit below lo
void hxq_host_pick(int lo, const unsigned long long *hist, unsigned long long *prefix,
                   unsigned long long *rem);
double hxq_key_to_double(unsigned long long key);
}  // namespace hx
