// liw_lm_rules.hpp — what Ceres' trust-region Levenberg-Marquardt minimizer (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
// default options) decides about a candidate step, stated once for every LM loop of the library: the step kernels (k_lm.hip,
// k_lm_quad.hip) and the host loop of the pose graph (k_posegraph.hip).  Pure functions of scalars, no HIP include: the file compiles
// with a host compiler alone (tests/cpp/lm_rules_driver.cpp replays the oracle's iteration records through it).  What a caller does
// around a rule — which lane stores, reductions, early returns — stays with the caller.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LIW_HD __host__ __device__ __forceinline__
#else
#define LIW_HD inline __attribute__((always_inline))
#endif

namespace liw {

constexpr double kMinDiag = 1e-6, kMaxDiag = 1e32, kMinRelDec = 1e-3, kFuncTol = 1e-6, kGradTol = 1e-10, kParamTol = 1e-8;
constexpr double kMaxRadius = 1e16, kMinRadius = 1e-32, kInitRadius = 1e4;
constexpr int kMaxInvalidSteps = 5;                          // max_num_consecutive_invalid_steps
constexpr double kFailedEvalCost = 1.7976931348623157e308;   // candidate cost of a failed evaluation (numeric_limits<double>::max())

// Termination codes (liw_summary::termination): 1 gradient, 2 function, 3 parameter tolerance, 4 iteration cap, 5 min radius, 6 FAILURE.

// ParameterToleranceReached, then FunctionToleranceReached, on an evaluated candidate: 3 / 2, or 0 = go on to rho.
// (A failed evaluation enters as kFailedEvalCost: far from x_cost, so it is rejected through rho, not terminated.)
LIW_HD int lm_candidate_term(double cand_step_norm, double x_norm, double x_cost, double cand_cost) {
    if (cand_step_norm <= kParamTol * (x_norm + kParamTol)) return 3;
    if (std::fabs(x_cost - cand_cost) <= kFuncTol * x_cost) return 2;
    return 0;
}

// IsStepSuccessful: relative_decrease > min_relative_decrease
LIW_HD bool lm_accepts(double rho) { return rho > kMinRelDec; }

// StepAccepted(rho): radius / max(1/3, 1 - (2 rho - 1)^3), capped; the cube by two multiplications (pow() is 200 instructions of a wave)
LIW_HD void lm_step_accepted(double rho, double& radius, double& dec, int& reuse) {
    const double t3 = 2.0 * rho - 1.0;
    radius = radius / std::fmax(1.0 / 3.0, 1.0 - t3 * t3 * t3);
    radius = std::fmin(kMaxRadius, radius);
    dec = 2.0; reuse = 0;
}

// StepRejected / StepIsInvalid: radius / decrease_factor, the factor doubles, the LM diagonal is kept
LIW_HD void lm_step_rejected(double& radius, double& dec, int& reuse) {
    radius = radius / dec; dec *= 2.0; reuse = 1;
}

// GradientToleranceReached (iteration zero, and after a successful step only: an unsuccessful one leaves the gradient as it was),
// then MinTrustRegionRadiusReached: 1 / 5 / 0.  The caller states `radius > kMinRadius` in the form it holds the radius in.
LIW_HD int lm_gradient_term(bool first, bool last_successful, double gmax, bool radius_above_min) {
    int term = 0;
    if (first) { if (gmax <= kGradTol) term = 1; }
    else if (last_successful && gmax <= kGradTol) term = 1;
    if (!term && !radius_above_min) term = 5;
    return term;
}

// MaxSolverIterationsReached; `fresh`: this pass evaluated iteration zero (so iteration == 0), which is not held against the cap
LIW_HD bool lm_cap_reached(int iteration, int max_iters, bool fresh) { return iteration >= max_iters && !fresh; }

// ComputeTrustRegionStep: the step is valid if the linear solve succeeded and the model predicts a finite decrease
LIW_HD bool lm_step_valid(bool solved, double model_cost_change) { return solved && model_cost_change > 0.0 && std::isfinite(model_cost_change); }

// HandleInvalidStep: FAILURE once this invalid step is the kMaxInvalidSteps-th in a row
LIW_HD bool lm_gives_up(int invalid_steps_before) { return invalid_steps_before + 1 >= kMaxInvalidSteps; }

}  // namespace liw
