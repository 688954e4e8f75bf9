// ctypes surface of csrc/sweep_plan.hpp for tests/test_sweep_plan_host.py: one function per plan, results as flat int64 arrays.
#include <string.h>

#include "../coordinatedescent.jl_amd/csrc/sweep_plan.hpp"

extern "C" {

int64_t sp_c_const(const char* name) {
#define K(x) if (!strcmp(name, #x)) return (int64_t)(x)
    K(kSpBlock); K(kSpUnroll); K(kSpNSum); K(kSpColGroup); K(kSpGramWaves); K(kSpGramChunk);
    K(kStepGridPerCU); K(kMaxStepGrid); K(kBlockGridPerCU); K(kSpColChunks); K(kSpColBatch); K(kColFillPerCU); K(kMaxBlockB);
    K(kShortRounds); K(kGramGridPerCU); K(kGram32GridPerCU); K(kLtGridPerCU); K(kLtLongRows); K(kWide64Rows);
    K(kInitGridCap); K(kWeightsGridCap); K(kMomentsGridCap);
#undef K
    return -1;
}
int64_t sp_c_gram_rec(int NG) { return sp_gram_rec(NG); }
int64_t sp_c_block_rec(int B) { return sp_block_rec(B); }

// out: ld, nvec, cap, blockB, cus, step_grid, block_grid, gram_units, partials_doubles
void sp_c_sizes(int f64, int64_t n, int64_t p, int cus, int64_t* out) {
    const SweepSizes s = sweep_sizes(f64 != 0, n, p, cus);
    const int64_t v[9] = {s.ld, s.nvec, s.cap, s.blockB, s.cus, s.step_grid, s.block_grid, s.gram_units, (int64_t)s.partials_doubles};
    memcpy(out, v, sizeof v);
}
// out: variant, cvn, nchunks, grid, rounds
void sp_c_gram(int64_t nvec, int64_t n, int cus, int NG, int esz, int lt, int ks, int64_t* out) {
    const GramPlan g = gram_plan(nvec, n, cus, NG, esz, lt, ks);
    const int64_t v[5] = {(int64_t)g.variant, g.cvn, g.nchunks, g.grid, g.rounds};
    memcpy(out, v, sizeof v);
}
int sp_c_gram_read_grid(int64_t nvec, int cus) { return gram_read_grid(nvec, cus); }
int sp_c_elementwise_grid(int64_t nvec, int64_t cap) { return elementwise_grid(nvec, cap); }
// out: groups, chunks, doubles
void sp_c_col_dots(int64_t bc, int64_t nvec, int cus, int width, int64_t* out) {
    const ColDotsPlan c = col_dots_plan(bc, nvec, cus, width);
    out[0] = c.groups; out[1] = c.chunks; out[2] = (int64_t)c.doubles;
}
// out: blocked, graph_worth, key, rewrites
void sp_c_route(int block_mode, int B, int has_w, int m, unsigned xbits, int dup, uint64_t* out) {
    const ChunkRoute r = chunk_route(block_mode != 0, B, has_w != 0, m, xbits, dup != 0);
    out[0] = r.blocked; out[1] = r.graph_worth; out[2] = r.key; out[3] = (uint64_t)r.rewrites;
}
void sp_c_traffic(int blocked, int B, int m, int has_w, const double* hs, int64_t n, int64_t esz, int64_t* launches, double* bytes) {
    const ChunkTraffic t = chunk_traffic(blocked != 0, B, m, has_w != 0, hs, n, (size_t)esz);
    *launches = t.launches; *bytes = t.bytes;
}

}  // extern "C"
