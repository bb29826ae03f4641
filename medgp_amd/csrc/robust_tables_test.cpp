// robust_tables_test.cpp -- CPU test of robust_tables.h (plain C++, host compiler, sanitizers; no GPU, no HIP): the digamma function
// against values computed at 40 digits, C(nu) against the same, the table layout, and the argument checks.
#include "robust_tables.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);          \
            if (++fails > 20) std::exit(1);                                   \
        }                                                                     \
    } while (0)

int main() {
    // psi(x) at 40 digits (rounded to 20)
    const double psi[][2] = {{0.01, -100.56088545786867242}, {0.5, -1.9635100260214234794}, {1.0, -0.57721566490153286061},
                             {1.5, 0.036489973978576520559}, {2.0, 0.42278433509846713939}, {3.25, 1.0169909110681790364},
                             {10.0, 2.2517525890667211076}, {12.0, 2.4426616799758120167}, {25.5, 3.2189424728839197665},
                             {100.5, 4.6051743525818452119}, {5e8, 20.030118655386465846}};
    for (const auto &p : psi) {
        const double got = robust_digamma(p[0]), tol = 8 * std::numeric_limits<double>::epsilon() * std::fmax(std::fabs(p[1]), 1.0);
        if (!(std::fabs(got - p[1]) <= tol)) std::printf("psi(%g) = %.17g, expected %.17g\n", p[0], got, p[1]);
        CHECK(std::fabs(got - p[1]) <= tol);
    }
    // C(nu) at 40 digits.  It is a difference of lgamma values of size ~ c log c: the tolerance is 16 eps of that size
    const double cst[][2] = {{0.1, 1.7598246082027130796}, {1.0, -0.08106146679532725822}, {2.0, -0.77102010020250820469},
                             {3.0, -1.3426855386776011765}, {4.5, -2.1430334313934604605}, {8.0, -3.9388062606007163648},
                             {30.0, -14.983425954069468598}, {1000.0, -499.99950008333335827}, {1e9, -499999999.9999999995}};
    for (const auto &p : cst) {
        const double c = p[0] / 2, size = std::fmax(std::fabs(std::lgamma(c)) + c, 1.0);
        const double got = robust_const(p[0]), tol = 16 * std::numeric_limits<double>::epsilon() * size;
        if (!(std::fabs(got - p[1]) <= tol)) std::printf("C(%g) = %.17g, expected %.17g (tol %g)\n", p[0], got, p[1], tol);
        CHECK(std::fabs(got - p[1]) <= tol);
    }
    // kappa(nu, 1) = C(nu) + c -> 0 as nu grows
    CHECK(std::fabs(robust_const(1e9) + 5e8) < 1e-4);
    // the table: [count][nu | c | C], entry (pos, d) of D covariates at robust_tab_at
    const int nbatch = 3, D = 4;
    std::vector<double> nu((size_t)nbatch * D), tab((size_t)nbatch * D * ROBUST_TAB, -1.0);
    for (size_t i = 0; i < nu.size(); i++) nu[i] = 1.0 + 0.5 * (double)i;
    robust_fill_table(nu.data(), (int64_t)nu.size(), tab.data());
    std::vector<int> seen(tab.size(), 0);
    for (int b = 0; b < nbatch; b++)
        for (int d = 0; d < D; d++) {
            const double v = nu[(size_t)b * D + d];
            for (int k = 0; k < ROBUST_TAB; k++) {
                const size_t at = robust_tab_at(b, D, d, k);
                CHECK(at < tab.size());
                if (at < tab.size()) seen[at]++;
            }
            CHECK(tab[robust_tab_at(b, D, d, ROBUST_TAB_NU)] == v);
            CHECK(tab[robust_tab_at(b, D, d, ROBUST_TAB_C)] == v / 2);
            CHECK(tab[robust_tab_at(b, D, d, ROBUST_TAB_CONST)] == robust_const(v));
        }
    for (int s : seen) CHECK(s == 1);
    // the argument checks
    CHECK(robust_nu_ok(1e-3) && robust_nu_ok(1e9));
    CHECK(!robust_nu_ok(0.0) && !robust_nu_ok(-1.0) && !robust_nu_ok(std::numeric_limits<double>::infinity()));
    CHECK(!robust_nu_ok(std::numeric_limits<double>::quiet_NaN()));
    const double bad[4] = {3.0, 4.0, 0.0, std::numeric_limits<double>::quiet_NaN()};
    CHECK(robust_first_bad_nu(bad, 2) == -1 && robust_first_bad_nu(bad, 4) == 2 && robust_first_bad_nu(bad, 0) == -1);
    CHECK(ROBUST_MAX_SWEEPS == 64);
    if (fails) { std::printf("robust_tables_test: %d FAILED\n", fails); return 1; }
    std::printf("robust_tables_test: ok\n");
    return 0;
}
