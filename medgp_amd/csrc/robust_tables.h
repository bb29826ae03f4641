// robust_tables.h -- host-only side of medgp_robust_nlml_grad (kernels_hetero.h): Student-t noise as a Gaussian scale mixture,
//   eps_i | tau_i ~ N(0, sigma^2_d / tau_i),  tau_i ~ Gamma(nu_d / 2, nu_d / 2),  q(tau_i) = Gamma(a_d, a_d s_i),  a_d = (nu_d + 1) / 2,
// whose negative evidence bound is the heteroscedastic nlml at the scales s plus sum_i kappa(nu_{m_i}, s_i) with
//   kappa(nu, s) = C(nu) + c (log s + 1 / s),   c = nu / 2,
//   C(nu) = psi(a) / 2 - lgamma(a) + lgamma(c) + c log(a / c) - a - (psi(a) - log a) / 2.
// The digamma and log-gamma values are formed HERE, once per entry and covariate, and travel to the device as a table; the device
// forms c (log s + 1 / s) and the sums.  Plain C++, no HIP: tested by robust_tables_test.cpp under sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#define ROBUST_MAX_SWEEPS 64
// the table of one (entry, covariate): nu | c = nu / 2 | C(nu); entries in the CALLER's order
#define ROBUST_TAB 3
enum { ROBUST_TAB_NU = 0, ROBUST_TAB_C = 1, ROBUST_TAB_CONST = 2 };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t robust_tab_at(int pos, int D, int d, int k) { return ((size_t)pos * D + d) * ROBUST_TAB + k; }

// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 12, then the asymptotic series through the x^-14 term (its
// first omitted term is below 4e-17 there)
inline double robust_digamma(double x) {
    double r = 0.0;
    while (x < 12.0) { r -= 1.0 / x; x += 1.0; }
    const double i2 = 1.0 / (x * x);
    const double series = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
    return r + ((std::log(x) - 0.5 / x) - series);
}

inline bool robust_nu_ok(double nu) { return std::isfinite(nu) && nu > 0.0; }
// index of the first nu of `count` that is not finite and > 0, or -1
inline int64_t robust_first_bad_nu(const double *nu, int64_t count) {
    for (int64_t i = 0; i < count; i++)
        if (!robust_nu_ok(nu[i])) return i;
    return -1;
}

inline double robust_const(double nu) {
    const double c = nu / 2, a = (nu + 1) / 2, psi = robust_digamma(a);
    return ((((psi / 2 - std::lgamma(a)) + std::lgamma(c)) + c * std::log(a / c)) - a) - (psi - std::log(a)) / 2;
}

// tab[count][ROBUST_TAB] from nu[count] (count = nbatch * D, the caller's order)
inline void robust_fill_table(const double *nu, int64_t count, double *tab) {
    for (int64_t i = 0; i < count; i++) {
        tab[i * ROBUST_TAB + ROBUST_TAB_NU] = nu[i];
        tab[i * ROBUST_TAB + ROBUST_TAB_C] = nu[i] / 2;
        tab[i * ROBUST_TAB + ROBUST_TAB_CONST] = robust_const(nu[i]);
    }
}
