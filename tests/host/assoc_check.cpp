// assoc_check.cpp -- a stand-alone check of the association scan's host code (assoc_layout.hpp,
// assoc_fit.hpp): no HIP, no library of the project.  Built with the host sanitizers by `make -C
// dbslmm_amd/csrc sanitize` (../bin/assoc_asan) and run by tests/test_assoc_host.py; also
// `g++ -std=c++17 assoc_check.cpp`.
//
// Design: the sample S under keep holes and non-finite values, Q^T Q = I, Q_0 = +-1 / sqrt(n), the
// residuals orthogonal to Q, yy, the layout of V (groups of 16 columns, zero rows outside S and in
// the padding, zero columns past the last) and the keep mask; the refusals (P = 0, df < 1, a
// rank-deficient W); df = 1 accepted.  Finish: every status on hand-made rows, a plain regression
// against its closed form, and the t tail at known values.  The first violation prints and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../dbslmm_amd/csrc/assoc_fit.hpp"
#include "../../dbslmm_amd/csrc/assoc_layout.hpp"

namespace {

std::string g_case;
#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        if (!(cond)) {                                                             \
            char msg_[512];                                                        \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);                              \
            fprintf(stderr, "assoc_check: %s: %s -- %s\n", g_case.c_str(), #cond, msg_); \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return static_cast<double>((g_rng * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
}

void check_design(const std::string& name, int32_t n_total, int32_t P, int32_t c1, bool holes) {
    g_case = name;
    const int64_t n_pad = (static_cast<int64_t>(n_total) + 255) / 256 * 256;
    std::vector<double> pheno(static_cast<size_t>(n_total) * P), covar(static_cast<size_t>(n_total) * c1);
    std::vector<uint8_t> keep(static_cast<size_t>(n_total), 1);
    for (double& v : pheno) v = rnd();
    for (double& v : covar) v = 3.0 + rnd();
    std::vector<uint8_t> in_s(static_cast<size_t>(n_total), 1);
    if (holes) {
        for (int32_t i : {3, 4, 15, 16, 63, 64, 65, 127, 128}) if (i < n_total) keep[i] = in_s[i] = 0;
        if (n_total > 20) { pheno[20 * P] = NAN; in_s[20] = 0; }
        if (n_total > 33 && c1 > 0) { covar[33 * c1 + c1 - 1] = INFINITY; in_s[33] = 0; }
    }
    assoc::Design d;
    const bool ok = assoc::build_design(n_total, n_pad, holes ? keep.data() : nullptr, pheno.data(), P,
                                        c1 ? covar.data() : nullptr, c1, d);
    CHECK(ok, "%s", d.err.c_str());
    int64_t n = 0;
    for (uint8_t s : in_s) n += s;
    const int32_t c = c1 + 1;
    CHECK(d.n == n && static_cast<int64_t>(d.sel.size()) == n, "n %lld want %lld", (long long)d.n, (long long)n);
    for (int64_t i = 0; i < n; ++i) CHECK(in_s[d.sel[i]] && (i == 0 || d.sel[i] > d.sel[i - 1]), "sel[%lld]", (long long)i);
    CHECK(d.n_cols == c1 + P && d.n_groups == (c1 + P + 15) / 16, "columns");
    CHECK(d.V.size() == static_cast<size_t>(d.n_groups) * n_pad * 16 && d.mask.size() == static_cast<size_t>(n_pad / 16), "sizes");
    for (int32_t a = 0; a < c; ++a)
        for (int32_t b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i) s += d.Q[a * n + i] * d.Q[b * n + i];
            CHECK(std::fabs(s - (a == b)) < 1e-12, "Q^T Q (%d, %d) = %g", a, b, s);
        }
    for (int64_t i = 0; i < n; ++i)
        CHECK(std::fabs(std::fabs(d.Q[i]) - 1.0 / std::sqrt(static_cast<double>(n))) < 1e-14, "Q_0[%lld] = %g", (long long)i, d.Q[i]);
    auto v = [&](int32_t col, int64_t i) { return d.V[(static_cast<size_t>(col / 16) * n_pad + i) * 16 + col % 16]; };
    for (int32_t col = 0; col < d.n_groups * 16; ++col) {
        std::vector<int64_t> rank(static_cast<size_t>(n_pad), -1);
        for (int64_t i = 0; i < n; ++i) rank[d.sel[i]] = i;
        double ss = 0.0;
        for (int64_t i = 0; i < n_pad; ++i) {
            const double x = v(col, i);
            if (col >= d.n_cols || rank[i] < 0) { CHECK(x == 0.0, "V(%d, %lld) = %g outside", col, (long long)i, x); continue; }
            if (col < c1) CHECK(x == d.Q[(col + 1) * n + rank[i]], "V(%d, %lld) is not Q", col, (long long)i);
            ss += x * x;
        }
        if (col >= c1 && col < d.n_cols) {
            CHECK(std::fabs(ss - d.yy[col - c1]) <= 1e-12 * ss, "yy[%d] = %g, |Yr|^2 = %g", col - c1, d.yy[col - c1], ss);
            for (int32_t a = 0; a < c; ++a) {
                double s = 0.0;
                for (int64_t i = 0; i < n; ++i) s += d.Q[a * n + i] * v(col, d.sel[i]);
                CHECK(std::fabs(s) < 1e-12 * std::sqrt(ss + 1.0), "Q_%d . Yr_%d = %g", a, col - c1, s);
            }
        }
    }
    for (int64_t i = 0; i < n_pad; ++i) {
        const uint32_t f = (d.mask[i / 16] >> (2 * (i % 16))) & 3u;
        CHECK(f == (i < n_total && in_s[i] ? 3u : 0u), "mask of individual %lld = %u", (long long)i, f);
    }
}

void check_refusals() {
    g_case = "refusals";
    assoc::Design d;
    std::vector<double> y(40), w(80);
    for (double& x : y) x = rnd();
    for (int i = 0; i < 40; ++i) { w[2 * i] = rnd(); w[2 * i + 1] = 2.0 * w[2 * i] - 1.0; }   // w1 = 2 w0 - 1: rank 2 of 3
    CHECK(!assoc::build_design(40, 256, nullptr, y.data(), 0, nullptr, 0, d) && !d.err.empty(), "P = 0 accepted");
    CHECK(!assoc::build_design(40, 256, nullptr, nullptr, 1, nullptr, 0, d), "null phenotypes accepted");
    CHECK(!assoc::build_design(40, 256, nullptr, y.data(), 1, w.data(), 2, d) && d.err.find("rank") != std::string::npos,
          "rank-deficient W accepted: %s", d.err.c_str());
    for (int i = 0; i < 40; ++i) w[2 * i + 1] = 0.5;                                           // a second intercept
    CHECK(!assoc::build_design(40, 256, nullptr, y.data(), 1, w.data(), 2, d), "constant covariate accepted");
    for (int i = 0; i < 40; ++i) w[2 * i + 1] = rnd();
    CHECK(assoc::build_design(40, 256, nullptr, y.data(), 1, w.data(), 2, d), "full rank refused: %s", d.err.c_str());
    // df = n - c - 1: 1 accepted, 0 refused (c = 3: n = 5 / 4 through keep)
    std::vector<uint8_t> keep(40, 0);
    for (int i = 0; i < 5; ++i) keep[7 * i] = 1;
    CHECK(assoc::build_design(40, 256, keep.data(), y.data(), 1, w.data(), 2, d) && d.n == 5, "df = 1 refused: %s", d.err.c_str());
    keep[0] = 0;
    CHECK(!assoc::build_design(40, 256, keep.data(), y.data(), 1, w.data(), 2, d), "df = 0 accepted");
    CHECK(!assoc::build_design(40, 100, nullptr, y.data(), 1, nullptr, 0, d), "n_pad no multiple of the stage accepted");
}

void check_finish() {
    g_case = "finish";
    // 10 individuals, c = 2 (one covariate column in V), P = 1
    const double yy[1] = {4.0};
    int32_t n_obs = 0;
    double af = 0, b = 0, se = 0, t = 0, p = 0;
    const double D[2] = {0.25, 0.5}, Mm[2] = {0.0, 0.0};
    // every call missing
    int32_t st = assoc::finish_row(10, 1, 1, 0, 0, 10, D, Mm, yy, &n_obs, &af, &b, &se, &t, &p, 1);
    CHECK(st == assoc::kNoCall && n_obs == 0 && std::isnan(af) && std::isnan(b) && std::isnan(p), "no call: %d", st);
    // all 0, all 1, all 2, all 2 with missing calls
    const int32_t mono[4][3] = {{0, 0, 0}, {10, 0, 0}, {0, 10, 0}, {0, 7, 3}};
    const double want_af[4] = {0.0, 0.5, 1.0, 1.0};
    for (int k = 0; k < 4; ++k) {
        st = assoc::finish_row(10, 1, 1, mono[k][0], mono[k][1], mono[k][2], D, Mm, yy, &n_obs, &af, &b, &se, &t, &p, 1);
        CHECK(st == assoc::kMonomorphic && n_obs == 10 - mono[k][2] && af == want_af[k] && std::isnan(b) && std::isnan(se) &&
                  std::isnan(t) && std::isnan(p), "monomorphic %d: status %d af %g", k, st, af);
    }
    // n1 = 4, n2 = 2: s1 = 8, s2 = 12, mu = 0.8, ssx = 12 - 6.4 = 5.6
    const double Dc[2] = {std::sqrt(5.6), 0.5};
    st = assoc::finish_row(10, 1, 1, 4, 2, 0, Dc, Mm, yy, &n_obs, &af, &b, &se, &t, &p, 1);
    CHECK(st == assoc::kCollinear && af == 0.4 && std::isnan(b), "collinear: %d", st);
    st = assoc::finish_row(10, 1, 1, 4, 2, 0, D, Mm, yy, &n_obs, &af, &b, &se, &t, &p, 1);
    {
        const double ssx = (12.0 + 0.8 * 0.8 * 0.0) - 0.8 * 0.8 * 10.0, xPx = ssx - 0.0625;
        const double wb = 0.5 / xPx, ws = std::sqrt((4.0 - wb * 0.5) / 7.0 / xPx);
        CHECK(st == assoc::kOk && n_obs == 10 && std::fabs(b - wb) <= 1e-15 && std::fabs(se - ws) <= 1e-15 &&
                  std::fabs(t - wb / ws) <= 1e-14, "ok row: %d %g %g %g", st, b, se, t);
        CHECK(std::fabs(p - assoc::student_t_two_sided(t, 7.0)) == 0.0 && p > 0.0 && p < 1.0, "p = %g", p);
    }
    // missing calls enter through Mm at the mean: t = D + mu Mm; Mm null: D is t itself
    const double Dm[2] = {0.25 - 0.75 * 0.2, 0.5 - 0.75 * 0.4}, Mk[2] = {0.2, 0.4};
    double b2 = 0, se2 = 0, t2 = 0, p2 = 0;
    st = assoc::finish_row(10, 1, 1, 2, 2, 2, Dm, Mk, yy, &n_obs, &af, &b, &se, &t, &p, 1);   // mu = 6 / 8
    const double tt[2] = {Dm[0] + 0.75 * Mk[0], Dm[1] + 0.75 * Mk[1]};
    const int32_t st2 = assoc::finish_row(10, 1, 1, 2, 2, 2, tt, nullptr, yy, &n_obs, &af, &b2, &se2, &t2, &p2, 1);
    CHECK(st == assoc::kOk && st2 == assoc::kOk && n_obs == 8 && af == 0.375 && b == b2 && se == se2 && t == t2 && p == p2,
          "Mm path: %g %g", b, b2);
    // two traits at stride 3
    double B[6], S[6], T[6], Pv[6];
    const double D3[3] = {0.25, 0.5, -0.3}, y2[2] = {4.0, 2.0};
    st = assoc::finish_row(10, 1, 2, 4, 2, 0, D3, nullptr, y2, &n_obs, &af, B, S, T, Pv, 3);
    CHECK(st == assoc::kOk && B[0] > 0 && B[3] < 0 && Pv[3] > 0, "two traits");
    // the t tail: t_1 is Cauchy, t_2 has a closed form; symmetric in t; NaN for non-finite input
    g_case = "t tail";
    const double pi = 3.14159265358979323846;
    for (double x : {1e-8, 0.5, 2.0, 10.0, 40.0}) {
        const double c1 = 1.0 - 2.0 / pi * std::atan(x), c2 = 1.0 - x / std::sqrt(2.0 + x * x);
        const double p1 = assoc::student_t_two_sided(x, 1.0), q2 = assoc::student_t_two_sided(-x, 2.0);
        CHECK(std::fabs(p1 - c1) <= 1e-10 * c1 + 1e-15, "df 1, t %g: %.17g want %.17g", x, p1, c1);
        CHECK(std::fabs(q2 - c2) <= 1e-10 * c2 + 1e-15, "df 2, t %g: %.17g want %.17g", x, q2, c2);
    }
    CHECK(assoc::student_t_two_sided(0.0, 5.0) == 1.0, "t = 0");
    CHECK(std::isnan(assoc::student_t_two_sided(NAN, 5.0)) && std::isnan(assoc::student_t_two_sided(INFINITY, 5.0)) &&
              std::isnan(assoc::student_t_two_sided(1.0, 0.0)) && std::isnan(assoc::student_t_two_sided(1.0, INFINITY)) &&
              std::isnan(assoc::student_t_two_sided(1.0, NAN)), "non-finite input");
    const double big = assoc::student_t_two_sided(3.0, 1e5);   // ~ the normal tail 0.0026998
    CHECK(std::fabs(big - 0.0027) < 2e-5, "df 1e5: %g", big);
}

}  // namespace

int main() {
    check_design("n 7, P 1", 7, 1, 0, false);
    check_design("n 65, c 3, P 2, holes", 65, 2, 2, true);
    check_design("n 257, 17 columns, holes", 257, 14, 3, true);
    check_design("n 300, 16 columns", 300, 1, 15, false);
    check_refusals();
    check_finish();
    printf("assoc_check: ok\n");
    return 0;
}
