// glm_weights_main.cpp -- the weight check of cdh_glm_set_weights (csrc/glm_plan.hpp: glm_first_bad_weight) as a stand-alone
// program, built by tests/test_glm_weights_host.py with g++ -fsanitize=address,undefined.  Every buffer is allocated at its
// exact length, so a read at or beyond n is the sanitizer's to report.  Prints "glm_weights_main OK <cases>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "glm_plan.hpp"

static int g_cases = 0;

static void expect(const std::vector<double>& v, int64_t want, const char* what) {
    // a heap copy of exactly n doubles (n = 0: no element is ever read)
    double* p = (double*)std::malloc(v.empty() ? 1 : v.size() * sizeof(double));
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    const int64_t got = glm_first_bad_weight(p, (int64_t)v.size());
    std::free(p);
    ++g_cases;
    if (got != want) {
        std::printf("FAIL %s: first bad weight %lld, expected %lld\n", what, (long long)got, (long long)want);
        std::exit(1);
    }
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double denorm = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();
    const double bad[] = {nan, inf, -inf, 0.0, -0.0, -1.0, -denorm};
    const double good[] = {1.0, denorm, 2.2250738585072014e-308, 1e-3, 1e3, big};
    for (int64_t n : {1, 2, 5, 64, 513}) {
        std::vector<double> v((size_t)n, 1.0);
        expect(v, n, "all ones");
        for (double g : good) {
            for (int64_t at : {(int64_t)0, n / 2, n - 1}) {
                std::vector<double> u = v;
                u[(size_t)at] = g;
                expect(u, n, "a good weight");
            }
        }
        for (double b : bad) {
            for (int64_t at : {(int64_t)0, n / 2, n - 1}) {
                std::vector<double> u = v;
                u[(size_t)at] = b;
                expect(u, at, "one bad weight");
                if (at + 1 < n) {                       // the FIRST of two is named
                    u[(size_t)(n - 1)] = nan;
                    expect(u, at, "two bad weights");
                }
            }
        }
    }
    expect({}, 0, "n = 0");
    std::printf("glm_weights_main OK %d\n", g_cases);
    return 0;
}
