// mbamd_rates.h -- category rates as a kernel argument (no host-to-device copy per beagleSetCategoryRates): the one type the
// kernels (mbamd_kernels.h, mbamd_f64.h) and the host runtime (RateSets, mbamd_host.h) share.
#pragma once

#define MBAMD_MAX_RATES 16
namespace mbamd {
struct RatesArg { double r[MBAMD_MAX_RATES]; };
}  // namespace mbamd
