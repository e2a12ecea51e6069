// ldsc_fit.hpp -- LD score regression on the host (host only, no HIP; dbslmm_ldsc_fit): the
// heritability the reference takes from an LDSC log (Rmd/Manual.Rmd:170).
// tests/host/ldsc_check.cpp checks it against fixed values under the host sanitizers.
//
// The rule (Bulik-Sullivan et al. 2015, as ldsc's Hsq applies it, one panel):
//   inputs   chi2_j = z_j^2, N_j, l_j (LD score), M; the intercept free, or fixed at a0.  chisq_max > 0
//            first drops the SNPs with chi2_j > chisq_max; n = the SNPs left.
//   model    Nbar = mean N, x_j = N_j l_j / Nbar.  Free: design [x, 1], y = chi2.  Fixed: design [x],
//            y = chi2 - a0.  P = 2 / 1 parameters; n < 2 P is too few SNPs.
//   start    h2 = M (mean chi2 - a) / mean(l N), a = 1 (free) or a0 (fixed)
//   weights  w_j = 1 / (2 (a + h2c N_j / M max(l_j, 1))^2) / max(l_j, 1), h2c = h2 clipped to [0, 1]
//            (the weight LD score is the regression LD score)
//   WLS      rows scaled by s_j = sqrt(w_j) / sum sqrt(w); normal equations A = sum (s X)(s X)^T,
//            b = sum (s X)(s y); coef = A^-1 b
//   rounds   two times: coef = WLS(w); h2 = coef_0 M / Nbar; a = coef_1 (free); w = weights(h2, a)
//   final    with the last w the per-block normal equations (A_b, b_b) of B = min(n_blocks, n)
//            contiguous blocks, block b = SNPs [floor(b n / B), floor((b + 1) n / B)) (integer
//            arithmetic; floor(linspace(0, n, B + 1))), formed once; A = sum A_b, b = sum b_b in
//            block order; est = A^-1 b is the estimate
//   SE       delete-one block jackknife: est_(-b) = (A - A_b)^-1 (b - b_b), pseudovalues
//            B est - (B - 1) est_(-b), SE = sqrt(var(pseudo, ddof 1) / B)
//   output   h2 = est_0 M / Nbar and its SE scaled alike; intercept = est_1 and its SE (free)
// A 2 x 2 system with |det| <= 1e-12 a11 a22 (1 x 1: a11 not > 0), or a non-finite entry, is
// singular.  No chi2 filter by default and no two-step estimator.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace ldsc {

enum { kOk = 0, kTooFew = 1, kSingular = 2 };

struct Result {
    double h2 = NAN, h2_se = NAN, intercept = NAN, intercept_se = NAN, mean_chi2 = NAN;
    int64_t n_used = 0;
    int32_t status = kOk;
};

// normal equations of P <= 2 parameters: a = {a11, a12, a22}, b = {b1, b2}
struct Normal {
    double a[3] = {0.0, 0.0, 0.0}, b[2] = {0.0, 0.0};
    void add(const Normal& o) {
        for (int k = 0; k < 3; ++k) a[k] += o.a[k];
        for (int k = 0; k < 2; ++k) b[k] += o.b[k];
    }
    Normal minus(const Normal& o) const {
        Normal r;
        for (int k = 0; k < 3; ++k) r.a[k] = a[k] - o.a[k];
        for (int k = 0; k < 2; ++k) r.b[k] = b[k] - o.b[k];
        return r;
    }
};

// coef = A^-1 b; false: singular
inline bool solve(const Normal& q, int P, double* coef) {
    if (P == 1) {
        if (!(q.a[0] > 0.0) || !std::isfinite(q.a[0]) || !std::isfinite(q.b[0])) return false;
        coef[0] = q.b[0] / q.a[0];
        coef[1] = 0.0;
        return true;
    }
    const double det = q.a[0] * q.a[2] - q.a[1] * q.a[1];
    if (!std::isfinite(det) || !std::isfinite(q.b[0]) || !std::isfinite(q.b[1]) ||
        !(std::fabs(det) > 1e-12 * q.a[0] * q.a[2]))
        return false;
    coef[0] = (q.a[2] * q.b[0] - q.a[1] * q.b[1]) / det;
    coef[1] = (q.a[0] * q.b[1] - q.a[1] * q.b[0]) / det;
    return true;
}

// fixed: intercept held at a0 (else free, a0 unused).  n_blocks >= 2.
inline Result fit(int64_t n_in, const double* chi2_in, const double* N_in, const double* l_in, double M,
                  bool fixed, double a0, int32_t n_blocks, double chisq_max) {
    Result R;
    std::vector<double> chi2, N, l;
    for (int64_t j = 0; j < n_in; ++j) {
        if (chisq_max > 0.0 && chi2_in[j] > chisq_max) continue;
        chi2.push_back(chi2_in[j]);
        N.push_back(N_in[j]);
        l.push_back(l_in[j]);
    }
    const int64_t n = static_cast<int64_t>(chi2.size());
    const int P = fixed ? 1 : 2;
    R.n_used = n;
    if (n < 2 * P) {
        R.status = kTooFew;
        return R;
    }
    double sN = 0.0, sc = 0.0, slN = 0.0;
    for (int64_t j = 0; j < n; ++j) {
        sN += N[j];
        sc += chi2[j];
        slN += l[j] * N[j];
    }
    const double dn = static_cast<double>(n), Nbar = sN / dn;
    R.mean_chi2 = sc / dn;
    std::vector<double> x(n), y(n), s(n);
    for (int64_t j = 0; j < n; ++j) {
        x[j] = N[j] * l[j] / Nbar;
        y[j] = fixed ? chi2[j] - a0 : chi2[j];
    }
    double a = fixed ? a0 : 1.0;
    double h2 = M * (R.mean_chi2 - a) / (slN / dn);
    // s_j = sqrt(w_j) / sum sqrt(w) of the current (h2, a)
    auto scales = [&]() {
        const double h2c = std::fmin(std::fmax(h2, 0.0), 1.0);
        double tot = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            const double lj = std::fmax(l[j], 1.0);
            const double c = a + h2c * N[j] / M * lj;
            s[j] = std::sqrt(1.0 / (2.0 * (c * c)) / lj);
            tot += s[j];
        }
        for (int64_t j = 0; j < n; ++j) s[j] /= tot;
    };
    auto normal = [&](int64_t j0, int64_t j1) {
        Normal q;
        for (int64_t j = j0; j < j1; ++j) {
            const double xs = x[j] * s[j], ys = y[j] * s[j];
            q.a[0] += xs * xs;
            q.b[0] += xs * ys;
            if (!fixed) {
                q.a[1] += xs * s[j];
                q.a[2] += s[j] * s[j];
                q.b[1] += s[j] * ys;
            }
        }
        return q;
    };
    double coef[2];
    scales();
    for (int round = 0; round < 2; ++round) {
        if (!solve(normal(0, n), P, coef)) {
            R.status = kSingular;
            return R;
        }
        h2 = coef[0] * M / Nbar;
        if (!fixed) a = coef[1];
        scales();
    }
    const int64_t B = n_blocks < n ? n_blocks : n;
    std::vector<Normal> blk(static_cast<size_t>(B));
    Normal tot;
    for (int64_t b = 0; b < B; ++b) {
        blk[static_cast<size_t>(b)] = normal(b * n / B, (b + 1) * n / B);
        tot.add(blk[static_cast<size_t>(b)]);
    }
    double est[2];
    if (!solve(tot, P, est)) {
        R.status = kSingular;
        return R;
    }
    std::vector<double> pseudo(static_cast<size_t>(2 * B));
    const double dB = static_cast<double>(B);
    for (int64_t b = 0; b < B; ++b) {
        double del[2];
        if (!solve(tot.minus(blk[static_cast<size_t>(b)]), P, del)) {
            R.status = kSingular;
            return R;
        }
        for (int k = 0; k < 2; ++k) pseudo[static_cast<size_t>(2 * b + k)] = dB * est[k] - (dB - 1.0) * del[k];
    }
    double se[2];
    for (int k = 0; k < 2; ++k) {
        double mean = 0.0, var = 0.0;
        for (int64_t b = 0; b < B; ++b) mean += pseudo[static_cast<size_t>(2 * b + k)];
        mean /= dB;
        for (int64_t b = 0; b < B; ++b) {
            const double d = pseudo[static_cast<size_t>(2 * b + k)] - mean;
            var += d * d;
        }
        se[k] = std::sqrt(var / (dB - 1.0) / dB);
    }
    R.h2 = est[0] * M / Nbar;
    R.h2_se = se[0] * M / Nbar;
    if (fixed) {
        R.intercept = a0;
        R.intercept_se = 0.0;
    } else {
        R.intercept = est[1];
        R.intercept_se = se[1];
    }
    return R;
}

}  // namespace ldsc
