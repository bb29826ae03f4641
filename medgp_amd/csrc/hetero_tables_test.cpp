// hetero_tables_test.cpp -- CPU test of hetero_tables.h (plain C++, host compiler, sanitizers; no GPU, no HIP): the roles of the call's
// vector buffer do not overlap and every index the kernels form through the element maps stays inside its role; the caller's packed
// rows and the grouped rows of an entry map onto each other exactly; the scale check accepts [2^-40, 2^40] and names the first
// offender; the capacity rule.
#include "hetero_tables.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

static int fails = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);          \
            if (++fails > 20) std::exit(1);                                   \
        }                                                                     \
    } while (0)

static int roundup(int x, int m) { return (x + m - 1) / m * m; }

// a plan of size classes as layout_plan makes them: entries sorted into classes of one leading dimension, laid out one behind the other
struct Cls { int count, ld; size_t off_vec; };

static void walk_roles(const std::vector<int> &ns, size_t vec0) {
    // one class per distinct padded size
    std::vector<Cls> cls;
    size_t need = 0;
    for (int ld = 64; ld <= 512; ld += 64) {
        int cnt = 0;
        for (int n : ns) cnt += roundup(n > 0 ? n : 1, 64) == ld;
        if (cnt) { cls.push_back({cnt, ld, need}); need += (size_t)cnt * ld; }
    }
    const size_t stride = het_role_stride(vec0, need);
    const HeteroBuffers hb = hetero_buffers(vec0, need, (int)ns.size(), 0, 6);
    CHECK(hb.vec_doubles == (size_t)HET_VECS * stride);
    CHECK(hb.tab_doubles == 6 * ns.size() && hb.delta_doubles == ns.size() && hb.out_doubles == 3);
    std::vector<unsigned char> seen(hb.vec_doubles, 0);
    for (int r = 0; r < HET_VECS; r++)
        for (const Cls &k : cls)
            for (int e = 0; e < k.count; e++)
                for (int i = 0; i < k.ld; i++) {
                    const size_t at = het_vec_offset(r, stride) + vec0 + k.off_vec + het_vec_at(e, k.ld, i);
                    CHECK(at < seen.size());
                    CHECK(at >= het_vec_offset(r, stride) && at < het_vec_offset(r + 1, stride));
                    if (at < seen.size()) { CHECK(seen[at] == 0); seen[at] = 1; }
                }
}

static void walk_rows() {
    // a patient of n = 7 rows on 3 covariates in an interleaved order: perm = the stable grouping
    const int meta[7] = {2, 0, 1, 0, 2, 1, 0};
    std::vector<int> perm;
    for (int d = 0; d < 3; d++)
        for (int i = 0; i < 7; i++)
            if (meta[i] == d) perm.push_back(i);
    const double src[7] = {10, 11, 12, 13, 14, 15, 16};
    double grouped[64];
    het_rows_to_grouped(src, perm.data(), 7, 64, grouped);
    const double want[7] = {11, 13, 16, 12, 15, 10, 14};
    for (int i = 0; i < 7; i++) CHECK(grouped[i] == want[i]);
    for (int i = 7; i < 64; i++) CHECK(grouped[i] == 1.0);
    double back[7];
    het_rows_to_caller(grouped, perm.data(), 7, true, back);
    for (int i = 0; i < 7; i++) CHECK(back[i] == src[i]);
    het_rows_to_caller(grouped, perm.data(), 7, false, back);
    for (int i = 0; i < 7; i++) CHECK(back[i] != back[i]);
    // n = 0: nothing is read or written but the padding
    het_rows_to_grouped(nullptr, nullptr, 0, 64, grouped);
    CHECK(grouped[0] == 1.0 && grouped[63] == 1.0);
    het_rows_to_caller(grouped, nullptr, 0, true, nullptr);
    const int en[4] = {3, 0, 65, 130};
    const std::vector<int64_t> off = het_row_offsets(en, 4);
    CHECK(off.size() == 5 && off[0] == 0 && off[1] == 3 && off[2] == 3 && off[3] == 68 && off[4] == 198);
}

static void check_scales() {
    CHECK(het_scale_ok(1.0) && het_scale_ok(HET_SCALE_MIN) && het_scale_ok(HET_SCALE_MAX));
    CHECK(HET_SCALE_MIN == std::ldexp(1.0, -40) && HET_SCALE_MAX == std::ldexp(1.0, 40));
    CHECK(!het_scale_ok(0.0) && !het_scale_ok(-1.0) && !het_scale_ok(std::nextafter(HET_SCALE_MIN, 0.0)));
    CHECK(!het_scale_ok(std::nextafter(HET_SCALE_MAX, 1e300)));
    CHECK(!het_scale_ok(std::numeric_limits<double>::quiet_NaN()) && !het_scale_ok(std::numeric_limits<double>::infinity()));
    const double s[5] = {1.0, 0.5, 8.0, -2.0, 0.0};
    CHECK(het_first_bad_scale(s, 3) == -1 && het_first_bad_scale(s, 5) == 3 && het_first_bad_scale(s, 0) == -1);
}

static void check_capacity() {
    // two matrices of 1000 doubles and three vectors of 10 under a budget of 2030 doubles: fits; one double less does not
    CHECK(hetero_fits(1000, 10, 2030 * sizeof(double)));
    CHECK(!hetero_fits(1000, 10, 2029 * sizeof(double)));
    CHECK(!hetero_fits(1000, 0, 1999 * sizeof(double)));
    CHECK(hetero_fits(0, 0, 0));
    CHECK(het_out_mean(5) == 0 && het_out_var(5) == 5);
}

int main() {
    walk_roles({3, 64, 65, 130}, 0);
    walk_roles({1}, 0);
    walk_roles({64, 64, 200, 512, 7}, 4096);
    walk_rows();
    check_scales();
    check_capacity();
    if (fails) { std::printf("hetero_tables_test: %d FAILED\n", fails); return 1; }
    std::printf("hetero_tables_test: ok\n");
    return 0;
}
