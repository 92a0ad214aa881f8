// The two-sided normal tail the Wald tests and the 1-df chi-square tests share (logit_kernel of ldx_logit.hip, firth_kernel of
// ldx_firth.hip, model_kernel of ldx_qc.hip): written once, so that the three report the same bits for the same statistic.
#pragma once

#include <math.h>

#include "ldx_common.h"

namespace ldx {

constexpr double kTailLn10 = 2.302585092994046;
constexpr double kTailSqrtHalf = 0.7071067811865476;

// ln p and p of the two-sided normal tail of z: p = erfc(|z| / sqrt 2); ln p from erfcx where erfc loses its range
__device__ __forceinline__ void normal_tail(double z, double &pv, double &nlp)
{
    const double t = fabs(z) * kTailSqrtHalf;
    pv = erfc(t);
    const double lnp = t < 5.0 ? log(pv) : log(erfcx(t)) - t * t;
    nlp = t == 0.0 ? 0.0 : -lnp / kTailLn10;
}

}  // namespace ldx
