// assoc_fit.hpp -- the per-row finish of the association scan (dbslmm_assoc; no HIP header needed): the
// Wald test of one SNP row of a linear model with covariates, from exact integer counts and the
// row's products with the residualised design (assoc_layout.hpp).  The same inline functions run in
// the finish kernel (assoc.hip) and on the host (dbslmm_assoc_stat_host, dbslmm_student_t_two_sided).
// tests/host/assoc_check.cpp checks them under the host sanitizers.
//
// The model ("Association scan"): S = the kept individuals, n = |S|; W (n x c) the
// covariates with the intercept first, Q its orthonormal basis, Yr = Y - Q Q^T Y, yy_p = |Yr_p|^2,
// V = [Q_1 .. Q_{c-1} | Yr].  Per row, over S: n1 / n2 = calls with dosage 1 / 2, nm = missing calls
// (readSNPIm's decode: 00 -> 2, 10 -> 1, 11 -> 0, 01 -> missing);
//   n_obs = n - nm, mu = (n1 + 2 n2) / n_obs, af = mu / 2
//   t_k   = D_k + mu Mm_k      (D = sum over observed calls of g V_k, Mm = sum over missing calls of V_k:
//                               the mean-imputed row's product with column k of V)
//   ssx   = (n1 + 4 n2) + mu^2 nm - mu^2 n            (the centring from the integers)
//   xPx   = ssx - sum_{k < c-1} t_k^2,  xPy = t_{c-1+p}
//   beta  = xPy / xPx, s2 = (yy_p - beta xPy) / df, se = sqrt(s2 / xPx), T = beta / se, df = n - c - 1
//   p     = 2 P(t_df <= -|T|)
// Status: kNoCall (n_obs = 0), kMonomorphic ((n1 + 4 n2) n_obs == (n1 + 2 n2)^2, in integers),
// kCollinear (xPx <= 1e-12 ssx); beta, se, T, p are NaN unless kOk, the integers are always reported.
// Every fp64 operation below is written out one rounding at a time (no contraction into FMAs), so
// the device and the host form the same bits from the same inputs, the library functions of the
// t tail (lgamma, log, log1p, exp) aside.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define ASSOC_HD __host__ __device__
#else
#define ASSOC_HD
#endif
#if defined(__clang__)
#define ASSOC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ASSOC_NO_CONTRACT
#endif

namespace assoc {

enum { kOk = 0, kNoCall = 1, kMonomorphic = 2, kCollinear = 3 };
constexpr double kCollinearTol = 1e-12;

// ln B(a, 1/2) = lgamma(a) + lgamma(1/2) - lgamma(a + 1/2).  Past a = 30 the two large lgammas (each
// rounded at its own magnitude, ~a ln a) would leave an absolute error of ~a ln a 2^-53 in their
// difference; there the difference comes from its asymptotic series (next term 31 / (12288 a^9)).
ASSOC_HD inline double ln_beta_half(double a) {
    ASSOC_NO_CONTRACT
    constexpr double kLnSqrtPi = 0.57236494292470008707;
    if (a < 30.0) return (::lgamma(a) + kLnSqrtPi) - ::lgamma(a + 0.5);
    const double r = 1.0 / a, r2 = r * r;
    const double s = r * (-1.0 / 8.0 + r2 * (1.0 / 192.0 + r2 * (-1.0 / 640.0 + r2 * (17.0 / 14336.0))));
    return kLnSqrtPi - (0.5 * ::log(a) + s);
}

// the continued fraction of the regularised incomplete beta I_x(a, b) (modified Lentz), for
// x < (a + 1) / (a + b + 2)
ASSOC_HD inline double beta_cf(double a, double b, double x) {
    ASSOC_NO_CONTRACT
    constexpr double kTiny = 1e-300, kEps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (::fabs(d) < kTiny) d = kTiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 20000; ++m) {
        const double dm = static_cast<double>(m), m2 = 2.0 * dm;
        double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (::fabs(d) < kTiny) d = kTiny;
        c = 1.0 + aa / c;
        if (::fabs(c) < kTiny) c = kTiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (::fabs(d) < kTiny) d = kTiny;
        c = 1.0 + aa / c;
        if (::fabs(c) < kTiny) c = kTiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (::fabs(del - 1.0) <= kEps) break;
    }
    return h;
}

// 2 P(t_df <= -|t|) = I_x(df / 2, 1 / 2), x = df / (df + t^2).  NaN for a non-finite t or df, or df <= 0.
ASSOC_HD inline double student_t_two_sided(double t, double df) {
    ASSOC_NO_CONTRACT
    if (!(::fabs(t) <= 1.79769313486231570815e308) || !(df > 0.0) || !(df <= 1.79769313486231570815e308))
        return __builtin_nan("");
    const double t2 = t * t;
    if (t2 == 0.0) return 1.0;
    if (!(t2 <= 1.79769313486231570815e308)) return 0.0;
    const double a = 0.5 * df, b = 0.5;
    const double q = t2 / df;
    const double x = 1.0 / (1.0 + q);              // df / (df + t^2)
    const double y = q / (1.0 + q);                // 1 - x, without the cancellation
    const double ln_x = -::log1p(q);
    const double ln_y = ::log(q) + ln_x;
    const double front = ::exp((a * ln_x + b * ln_y) - ln_beta_half(a));
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
    return 1.0 - front * beta_cf(b, a, y) / b;
}

// One row: the counts n1, n2, nm over the n kept individuals, D / Mm the c1 + P products of the
// row with V (Mm null: D holds t itself), yy the P residual sums of squares; c1 = c - 1.  Writes
// n_obs, af, and beta / se / tstat / p of trait q at [q * stride]; returns the status.
ASSOC_HD inline int32_t finish_row(int64_t n, int32_t c1, int32_t P, int32_t n1, int32_t n2, int32_t nm,
                                   const double* D, const double* Mm, const double* yy, int32_t* n_obs_out,
                                   double* af_out, double* beta, double* se, double* tstat, double* p,
                                   int64_t stride) {
    ASSOC_NO_CONTRACT
    const double nan = __builtin_nan("");
    const int64_t n_obs = n - nm;
    const int64_t s1 = static_cast<int64_t>(n1) + 2 * static_cast<int64_t>(n2);
    const int64_t s2 = static_cast<int64_t>(n1) + 4 * static_cast<int64_t>(n2);
    *n_obs_out = static_cast<int32_t>(n_obs);
    int32_t status = kOk;
    double mu = nan, ssx = nan, xPx = nan;
    if (n_obs <= 0) {
        status = kNoCall;
    } else {
        mu = static_cast<double>(s1) / static_cast<double>(n_obs);
        if (s2 * n_obs == s1 * s1) status = kMonomorphic;
    }
    *af_out = 0.5 * mu;
    if (status == kOk) {
        const double mu2 = mu * mu;
        ssx = (static_cast<double>(s2) + mu2 * static_cast<double>(nm)) - mu2 * static_cast<double>(n);
        xPx = ssx;
        for (int32_t k = 0; k < c1; ++k) {
            const double t = Mm ? D[k] + mu * Mm[k] : D[k];
            xPx = xPx - t * t;
        }
        if (!(xPx > kCollinearTol * ssx)) status = kCollinear;
    }
    const double df = static_cast<double>(n - c1 - 2);
    for (int32_t q = 0; q < P; ++q) {
        double b = nan, s = nan, ts = nan, pv = nan;
        if (status == kOk) {
            const double xPy = Mm ? D[c1 + q] + mu * Mm[c1 + q] : D[c1 + q];
            b = xPy / xPx;
            const double s2r = (yy[q] - b * xPy) / df;
            s = ::sqrt(s2r / xPx);
            ts = b / s;
            pv = student_t_two_sided(ts, df);
        }
        beta[q * stride] = b;
        se[q * stride] = s;
        tstat[q * stride] = ts;
        p[q * stride] = pv;
    }
    return status;
}

}  // namespace assoc
