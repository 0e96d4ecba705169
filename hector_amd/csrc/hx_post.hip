// hx_post.hip -- the device code of hx_member_score, hx_member_metrics, hx_member_pair_metrics, hx_ensemble_quantiles, the
// bin probabilities, the moment and Sobol sums, apart from the
// year-loop kernels of hx_kernels.hip (their object, and so their code generation, stays as it is).
#include "hx_dev_post.h"
