// What the design entry points share (obe_interest.hip: obe_variance_reduction; obe_design.hip: obe_design_step and
// obe_design_interest_step): the score for parameters of interest and the first-finite-maximum arg-max, each stated once
// next to its kernel and launched through these.  Internal to the library (hidden visibility): not part of the C ABI.
#pragma once

#include "obe_common.h"

namespace obe {

constexpr int kGainRows = 8;                       // rows one launch of the score serves: obe_output_covariance's

// variance_reduction_kernel (obe_interest.hip) over up to 8 rows: the arguments of obe_variance_reduction, which the
// caller has checked (n_rows 1..8, n_channels 1..OBE_MAX_CHANNELS, a grid of (n_settings + 255) / 256 workgroups).
int launch_variance_reduction(hipStream_t st, const double* d_ycov, const double* d_xcov, int n_rows, int n_channels,
                              int64_t n_settings, const double* d_noise_var, int64_t ld_noise, const double* d_pvar,
                              const double* h_weights, const double* d_cost, double cost, double* d_gain,
                              double* d_utility, int accumulate);

// design_best_kernel (obe_design.hip): d_best = (the largest finite utility of a setting that is not taken, the first
// index that has it).
int launch_design_best(hipStream_t st, const double* d_utility, int64_t n_settings, const uint8_t* d_taken, double* d_best);

}  // namespace obe
