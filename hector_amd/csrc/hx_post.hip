// hx_post.hip -- the device code of hx_member_score and hx_ensemble_quantiles, apart from the
// year-loop kernels of hx_kernels.hip (their object, and so their code generation, stays as it is).
#include "hx_dev_post.h"
