// assoc_layout.hpp -- the host part of the association scan (host only, no HIP; dbslmm_assoc): the
// sample S, the Householder QR of the covariates, the residualised phenotypes and the layout of V
// that the product kernel (assoc.hip) stages through LDS.  tests/host/assoc_check.cpp checks it under
// the host sanitizers.
//
//   S      the individuals with keep != 0 (keep null: all) whose phenotypes and covariates are all
//          finite; n = |S|.  df = n - c - 1 >= 1 or the design is refused.
//   W      n x c, column 0 the intercept (added here), then the caller's c - 1 covariates
//   Q      the orthonormal basis of W by Householder QR (column 0 = +-1 / sqrt(n) up to rounding);
//          |R_kk| <= 1e-10 |W_k| is a rank-deficient W: refused
//   Yr     Y - Q (Q^T Y), yy_p = |Yr_p|^2 (summed in individual order)
//   V      the columns [Q_1 .. Q_{c-1} | Yr_0 .. Yr_{P-1}] in groups of kAssocCols = 16: element
//          (group g, individual i, column k) at (g n_pad + i) 16 + k.  Rows of individuals outside S
//          (and of the image's padding, i >= n_total) and the columns past the last are zero, so a
//          product with V sums over S alone.
//   mask   per image dword (16 individuals) the 2-bit fields 11 of the individuals in S: what the
//          integer pass ANDs the image with.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

constexpr int kAssocCols = 16;           // columns of V per pass (one MFMA tile)
constexpr int kAssocRows = 16;           // panel rows per tile
constexpr int kAssocStage = 64;          // individuals per LDS stage (one 16-B image chunk per row)
constexpr int kAssocChunkIndiv = 4096;   // individuals per chunk (chunk_indiv = 0): a constant, never the machine's

namespace assoc {

struct Design {
    int64_t n = 0;                  // |S|
    int32_t c1 = 0, P = 0;          // covariates without the intercept, traits
    int32_t n_cols = 0, n_groups = 0;
    int64_t n_pad = 0;
    std::vector<int32_t> sel;       // S, ascending
    std::vector<double> Q;          // n x c, column-major (column 0 the intercept's)
    std::vector<double> V;          // [n_groups][n_pad][16]
    std::vector<double> yy;         // P
    std::vector<uint32_t> mask;     // n_pad / 16
    std::string err;                // why build_design returned false
};

// n_pad: the individuals of an image row (a multiple of kAssocStage, >= n_total).  pheno: n_total x P,
// covar: n_total x c1 (null when c1 = 0), both row-major.
inline bool build_design(int32_t n_total, int64_t n_pad, const uint8_t* keep, const double* pheno, int32_t P,
                         const double* covar, int32_t c1, Design& d) {
    d = Design();
    if (n_total < 1 || n_pad < n_total || n_pad % kAssocStage != 0) { d.err = "bad panel size"; return false; }
    if (P < 1 || !pheno) { d.err = "at least one phenotype is needed"; return false; }
    if (c1 < 0 || (c1 > 0 && !covar)) { d.err = "bad covariates"; return false; }
    d.c1 = c1;
    d.P = P;
    d.n_pad = n_pad;
    d.n_cols = c1 + P;
    d.n_groups = (d.n_cols + kAssocCols - 1) / kAssocCols;
    for (int32_t i = 0; i < n_total; ++i) {
        bool ok = !keep || keep[i] != 0;
        for (int32_t q = 0; ok && q < P; ++q) ok = std::isfinite(pheno[static_cast<int64_t>(i) * P + q]);
        for (int32_t k = 0; ok && k < c1; ++k) ok = std::isfinite(covar[static_cast<int64_t>(i) * c1 + k]);
        if (ok) d.sel.push_back(i);
    }
    const int64_t n = static_cast<int64_t>(d.sel.size());
    const int32_t c = c1 + 1;
    d.n = n;
    if (n - c - 1 < 1) { d.err = "too few individuals: n - c - 1 < 1"; return false; }
    // Householder QR of W in place (R in the upper triangle, the reflectors v_k below, v_k[k] kept apart)
    std::vector<double> A(static_cast<size_t>(n) * c), vk(static_cast<size_t>(c)), beta(static_cast<size_t>(c));
    auto a = [&](int64_t i, int32_t k) -> double& { return A[static_cast<size_t>(k) * n + i]; };
    for (int64_t i = 0; i < n; ++i) {
        a(i, 0) = 1.0;
        for (int32_t k = 0; k < c1; ++k) a(i, k + 1) = covar[static_cast<int64_t>(d.sel[i]) * c1 + k];
    }
    for (int32_t k = 0; k < c; ++k) {
        double norm0 = 0.0;                       // |W_k|, the whole original column
        for (int64_t i = 0; i < n; ++i) {
            const double w = k == 0 ? 1.0 : covar[static_cast<int64_t>(d.sel[i]) * c1 + (k - 1)];
            norm0 += w * w;
        }
        norm0 = std::sqrt(norm0);
        double s = 0.0;
        for (int64_t i = k; i < n; ++i) s += a(i, k) * a(i, k);
        const double nrm = std::sqrt(s);
        if (!(nrm > 1e-10 * norm0)) { d.err = "the covariates (with the intercept) are rank deficient"; return false; }
        const double alpha = a(k, k) > 0.0 ? -nrm : nrm;
        vk[k] = a(k, k) - alpha;                  // v = x - alpha e_k
        double vv = vk[k] * vk[k];
        for (int64_t i = k + 1; i < n; ++i) vv += a(i, k) * a(i, k);
        beta[k] = 2.0 / vv;
        for (int32_t j = k + 1; j < c; ++j) {
            double dot = vk[k] * a(k, j);
            for (int64_t i = k + 1; i < n; ++i) dot += a(i, k) * a(i, j);
            dot *= beta[k];
            a(k, j) -= dot * vk[k];
            for (int64_t i = k + 1; i < n; ++i) a(i, j) -= dot * a(i, k);
        }
        a(k, k) = alpha;
    }
    // Q = H_0 .. H_{c-1} [I_c; 0]
    d.Q.assign(static_cast<size_t>(n) * c, 0.0);
    auto q = [&](int64_t i, int32_t k) -> double& { return d.Q[static_cast<size_t>(k) * n + i]; };
    for (int32_t k = 0; k < c; ++k) q(k, k) = 1.0;
    for (int32_t k = c - 1; k >= 0; --k)
        for (int32_t j = 0; j < c; ++j) {
            double dot = vk[k] * q(k, j);
            for (int64_t i = k + 1; i < n; ++i) dot += a(i, k) * q(i, j);
            dot *= beta[k];
            q(k, j) -= dot * vk[k];
            for (int64_t i = k + 1; i < n; ++i) q(i, j) -= dot * a(i, k);
        }
    // V and yy
    d.V.assign(static_cast<size_t>(d.n_groups) * n_pad * kAssocCols, 0.0);
    auto v = [&](int32_t col, int64_t indiv) -> double& {
        return d.V[(static_cast<size_t>(col / kAssocCols) * n_pad + indiv) * kAssocCols + col % kAssocCols];
    };
    for (int32_t k = 1; k < c; ++k)
        for (int64_t i = 0; i < n; ++i) v(k - 1, d.sel[i]) = q(i, k);
    d.yy.assign(static_cast<size_t>(P), 0.0);
    std::vector<double> y(static_cast<size_t>(n)), coef(static_cast<size_t>(c));
    for (int32_t t = 0; t < P; ++t) {
        for (int64_t i = 0; i < n; ++i) y[i] = pheno[static_cast<int64_t>(d.sel[i]) * P + t];
        for (int32_t k = 0; k < c; ++k) {
            double dot = 0.0;
            for (int64_t i = 0; i < n; ++i) dot += q(i, k) * y[i];
            coef[k] = dot;
        }
        double ss = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double r = y[i];
            for (int32_t k = 0; k < c; ++k) r -= q(i, k) * coef[k];
            v(c1 + t, d.sel[i]) = r;
            ss += r * r;
        }
        d.yy[t] = ss;
    }
    d.mask.assign(static_cast<size_t>(n_pad / 16), 0u);
    for (int64_t i = 0; i < n; ++i) d.mask[d.sel[i] / 16] |= 3u << (2 * (d.sel[i] % 16));
    return true;
}

}  // namespace assoc
