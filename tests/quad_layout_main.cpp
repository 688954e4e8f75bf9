// A stand-alone program over csrc/quad_solve_types.hpp (tests/test_quad_host.py builds and runs it, with the host sanitizers):
// for every p given on the command line it checks that the per-problem LDS arrays of k_quad_solve do not overlap, are
// aligned for their element type and end inside the budget, and prints "p <p> bytes <n> fits <0|1>"; then "max_p <P>".
// Exit status 1 on the first violated property (with a line on stderr).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/quad_solve_types.hpp"

struct Arr { const char* name; size_t off, bytes, align; };

static int check(int64_t p) {
    const QuadLds L = quad_lds_layout(p);
    const size_t d = (size_t)p * sizeof(double), i = (size_t)p * sizeof(int32_t);
    const std::vector<Arr> a = {{"g", L.g, d, 8}, {"beta", L.beta, d, 8}, {"inv_a", L.inv_a, d, 8}, {"omega", L.omega, d, 8},
                                {"list", L.list, i, 4}, {"slot2ind", L.slot2ind, i, 4}, {"ind2slot", L.ind2slot, i, 4},
                                {"order", L.order, i, 4}, {"draw", L.draw, i, 4}, {"fyoff", L.fyoff, i + sizeof(int32_t), 4},
                                {"fybucket", L.fybucket, i, 4}, {"fypar", L.fypar, i, 4}};
    for (size_t x = 0; x < a.size(); ++x) {
        if (a[x].off % a[x].align) { fprintf(stderr, "p %lld: %s is misaligned\n", (long long)p, a[x].name); return 1; }
        if (a[x].off + a[x].bytes > L.end) { fprintf(stderr, "p %lld: %s runs past the end\n", (long long)p, a[x].name); return 1; }
        for (size_t y = x + 1; y < a.size(); ++y)
            if (a[x].off < a[y].off + a[y].bytes && a[y].off < a[x].off + a[x].bytes) {
                fprintf(stderr, "p %lld: %s and %s overlap\n", (long long)p, a[x].name, a[y].name);
                return 1;
            }
    }
    if (L.end != quad_lds_bytes(p) || L.end % 8) { fprintf(stderr, "p %lld: the total is inconsistent\n", (long long)p); return 1; }
    // touch every byte the layout claims, in a buffer of exactly that size (the sanitizer's bounds are the layout's)
    std::vector<unsigned char> lds(L.end, 0);
    for (const Arr& r : a) for (size_t b = 0; b < r.bytes; ++b) lds[r.off + b] += 1;
    for (const Arr& r : a) for (size_t b = 0; b < r.bytes; ++b) if (lds[r.off + b] != 1) { fprintf(stderr, "p %lld: a byte of %s is claimed twice\n", (long long)p, r.name); return 1; }
    printf("p %lld bytes %zu fits %d\n", (long long)p, L.end, L.end <= kQuadLdsBudget ? 1 : 0);
    return 0;
}

int main(int argc, char** argv) {
    for (int x = 1; x < argc; ++x) if (check(atoll(argv[x]))) return 1;
    printf("max_p %lld budget %zu\n", (long long)kQuadMaxP, kQuadLdsBudget);
    // the argument checks
    std::vector<unsigned char> seen(8, 0);
    const int64_t ok[] = {3, 1, 8}, twice[] = {3, 1, 3}, out[] = {3, 9};
    const bool checks = !quad_check_create(kQuadMaxP, 1) && quad_check_create(kQuadMaxP + 1, 1) && quad_check_create(0, 1) &&
                        quad_check_create(4, 0) && !quad_check_problem(0, 1) && quad_check_problem(1, 1) && quad_check_problem(-1, 1) &&
                        quad_check_problem(0, 0) && !quad_check_support(8, 3, ok, seen.data()) && quad_check_support(8, 3, twice, seen.data()) &&
                        quad_check_support(8, 2, out, seen.data()) && quad_check_support(8, 9, ok, seen.data()) &&
                        !quad_check_support(8, 3, ok, seen.data()) /* the scratch came back clean */ &&
                        !quad_check_options(10, 1, 0) && quad_check_options(10, 0, 0) && quad_check_options(10, 0, 64) &&
                        !quad_check_options(10, 0, 63) && quad_check_options(-1, 1, 50);
    if (!checks) { fprintf(stderr, "an argument check accepts or refuses the wrong thing\n"); return 1; }
    printf("message %s\n", quad_check_create(kQuadMaxP + 1, 1));
    return 0;
}
