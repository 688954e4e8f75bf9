// Stand-alone check of csrc/vc_gram_batch_types.hpp under the host sanitizers (tests/test_vc_gram_batch_host.py builds and
// runs it): the plan of a call over the sweep of (n, Q, mb, m) -- every point marked in an exactly-sized heap block by the
// group and share that own it, so that an edge out of range is an ASan report and a point owned twice or never a count; the
// records of a group inside the partial buffer, back to back; and the batch check on exactly-sized argument arrays, so
// that a read past the m-th point is an ASan report too.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../coordinatedescent.jl_amd/csrc/vc_gram_batch_types.hpp"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++fails; } \
    } while (0)

static void walk(int64_t n, int Q, int64_t mb, int64_t m) {
    const int64_t G = vc_gram_grid(n, Q, mb), nrec = vc_gram_rec(Q, mb).n, ngroups = vgb_groups(n, Q, mb, m);
    int* owners = (int*)std::calloc((size_t)m, sizeof(int));
    EXPECT(vgb_resident(n, Q, mb) == (vc_gram_chunks(n) <= G));
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t first = vgb_group_first(n, Q, mb, g), pts = vgb_group_size(n, Q, mb, m, g);
        const int64_t gy = vgb_grid_y(n, Q, mb, pts), per = vgb_share_points(n, Q, mb, pts);
        EXPECT(pts >= 1 && pts <= kVgbMaxGroupPoints && gy >= 1 && gy <= 65535);
        EXPECT(vgb_rec_offset(n, Q, mb, pts - 1, G - 1) + nrec <= kVgbPartialDoubles && pts * nrec <= kVgbOutDoubles);
        EXPECT(vgb_rec_offset(n, Q, mb, 0, 0) == 0 && vgb_rec_offset(n, Q, mb, pts - 1, G - 1) == (pts * G - 1) * nrec);
        EXPECT(vgb_share_begin(n, Q, mb, pts, 0) == 0 && vgb_share_begin(n, Q, mb, pts, gy) == pts);
        if (!vgb_resident(n, Q, mb)) EXPECT(per == 1 && gy == pts);
        for (int64_t s = 0; s < gy; ++s) {
            const int64_t b0 = vgb_share_begin(n, Q, mb, pts, s), b1 = vgb_share_begin(n, Q, mb, pts, s + 1);
            EXPECT(b0 < b1 && b1 - b0 <= per);                       // no empty share
            for (int64_t t = b0; t < b1; ++t) ++owners[first + t];
        }
    }
    EXPECT(vgb_group_size(n, Q, mb, m, ngroups) == 0);
    for (int64_t t = 0; t < m; ++t) EXPECT(owners[t] == 1);          // every point in exactly one group and one share
    std::free(owners);
}

int main() {
    const int64_t ns[] = {1, 64, 65, 32768, 32769, 1000000}, mbs[] = {1, 3, 4, 64};
    for (int64_t n : ns)
        for (int Q = 0; Q <= kVgMaxDegree; ++Q)
            for (int64_t mb : mbs) {
                const int64_t pg = vgb_group_points(n, Q, mb);
                EXPECT(pg >= 8);
                const int64_t ms[] = {1, 2, pg - 1, pg, pg + 1, kVgbMaxPoints};
                for (int64_t m : ms)
                    if (m >= 1 && m <= kVgbMaxPoints) walk(n, Q, mb, m);
            }
    // the batch check: m-entry heap arrays, one thing wrong at a time
    const int64_t m = 5;
    double* h = (double*)std::malloc(sizeof(double) * m);
    double* z0 = (double*)std::malloc(sizeof(double) * m);
    int64_t* lo = (int64_t*)std::malloc(sizeof(int64_t) * m);
    int64_t* idx = (int64_t*)std::malloc(sizeof(int64_t) * 3);
    auto reset = [&] {
        for (int64_t t = 0; t < m; ++t) { h[t] = 0.25 + 0.1 * (double)t; z0[t] = 0.1 * (double)t; lo[t] = t % 2 ? t : -1; }
        idx[0] = 3; idx[1] = 1; idx[2] = 3;
    };
    int64_t bad = 7;
    auto chk = [&](int64_t mm, const double* hh, const double* zz, const int64_t* ll) {
        return vc_gram_batch_check(1, true, true, 3, 10, 0, mm, hh, zz, ll, 1, 3, idx, &bad);
    };
    reset();
    EXPECT(chk(m, h, z0, lo) == nullptr && bad == -1);              // a mixed batch
    EXPECT(chk(m, h, z0, nullptr) == nullptr && bad == -1);
    EXPECT(chk(0, h, z0, lo) != nullptr && bad == -1);
    EXPECT(chk(kVgbMaxPoints + 1, h, z0, lo) != nullptr && bad == -1);
    EXPECT(chk(m, nullptr, z0, lo) != nullptr && bad == -1);
    EXPECT(chk(m, h, nullptr, lo) != nullptr && bad == 0);           // point 0 leaves no row out
    for (int64_t t = 0; t < m; ++t) lo[t] = t;
    EXPECT(chk(m, h, nullptr, lo) == nullptr && bad == -1);          // every point leaves a row out: z0 may be NULL
    reset();
    h[3] = 0.0;
    EXPECT(chk(m, h, z0, lo) != nullptr && bad == 3);
    reset();
    z0[2] = INFINITY;
    EXPECT(chk(m, h, z0, lo) != nullptr && bad == 2);
    reset();
    z0[1] = NAN;                                                     // point 1 leaves a row out: its z0 is not read as a point
    EXPECT(chk(m, h, z0, lo) == nullptr && bad == -1);
    lo[4] = 10;
    EXPECT(chk(m, h, z0, lo) != nullptr && bad == 4);
    reset();
    lo[0] = -2;
    EXPECT(chk(m, h, z0, lo) != nullptr && bad == 0);
    reset();
    idx[2] = 4;
    EXPECT(chk(m, h, z0, lo) != nullptr && bad == 0);
    std::free(h); std::free(z0); std::free(lo); std::free(idx);
    std::printf(fails ? "vc_gram_batch_main: %d FAILED\n" : "vc_gram_batch_main OK\n", fails);
    return fails ? 1 : 0;
}
