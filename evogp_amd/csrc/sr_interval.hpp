// sr_interval.hpp — the constants of the interval pass (sr_interval.hip).  tests/interval_ref.py holds the same table (E_ULPS, W_ULPS,
// W_DIV, TRIG_MAX, TRIG_MARGIN): the restatement is the definition, and the two are kept side by side.
#pragma once

namespace evogp {

// flag bits of an interval
constexpr unsigned kItvMayNan = 1u, kItvMalformed = 2u;

// E(f): the documented OCML bound of a library function in fp32 ulps (tests/ulp_bounds.py); W(f) = 2 E(f) + 1 is how far an
// endpoint taken from the function's own fp32 result moves outward: the library is not known to be monotone, so the error at the
// endpoint and the error at the inner point both count, and one more ulp covers the rounding of the true value between them.
constexpr int itv_widen(int e_ulps) { return 2 * e_ulps + 1; }
constexpr int kWSinCos = itv_widen(4);   // sin cos 4
constexpr int kWTan = itv_widen(5);      // tan 5
constexpr int kWHyp = itv_widen(5);      // sinh cosh tanh 5
constexpr int kWLogExp = itv_widen(3);   // log loose_log exp 3
constexpr int kWPow = itv_widen(16);     // pow loose_pow 16
// the divisions: the quotient of the endpoints is correctly rounded here, the threaded code's division is faithfully rounded (< 1 ulp)
constexpr int kWDiv = 1;

// the float64 tests that place the extrema of sin / cos and the poles of tan
constexpr double kItvPi = 3.141592653589793;
constexpr double kItvTwoPi = 2.0 * kItvPi;
constexpr double kItvHalfPi = 0.5 * kItvPi;
constexpr double kItvTrigMax = 1048576.0;                 // 2^20: beyond it the answer is the full range
constexpr double kItvTrigMargin = 9.5367431640625e-07;    // 2^-20 of a period: an endpoint this close to an extremum counts as on it

} // namespace evogp
