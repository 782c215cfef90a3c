// walk_prep.hip -- what a walk launch is handed ready-made (gfx950): the key shift of a shape, the rand_r stream position of every
// root (subgacc_rng_positions), the packed hop records of a graph (subgacc_hop_records_*) and the roots of a step of one source
// against K targets (subgacc_step_prologue_star, include/subgacc_star.h).  The walk kernels themselves:
// walk.hip (general), walk_pipe.hip, walk_rows.hip, walk_small.hip.
#include "common.hpp"
#include "../../include/subgacc_star.h"
#include "walk_common.hpp"
#include "uniq_table.hpp"
#include <stdlib.h>

namespace subgacc {

template <bool IDX64>
__global__ void rng_calls_kernel(const void *__restrict__ indptr, const int32_t *__restrict__ query, int64_t n,
                                 int64_t num_nodes, int M, int m, int wo, int cap, int32_t *__restrict__ calls) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t beg, deg = 0;
    if ((uint64_t)(int64_t)query[i] < (uint64_t)num_nodes) load_row<IDX64>(indptr, query[i], beg, deg);   // else: the walk kernel flags it
    if (cap && deg > kNeighCap) deg = kNeighCap;
    int32_t c = 0;
    if (deg > 0) c = wo ? ((deg > M ? M : 0) + M * (m - 1)) : M * m;
    calls[i] = c;
}

// libgomp static schedule: the first n%T threads own ceil(n/T) iterations
__global__ void rng_positions_kernel(const int64_t *__restrict__ calls_excl, int64_t n, int32_t streams,
                                     uint64_t calls_before, uint32_t seed, uint32_t *__restrict__ pos,
                                     uint32_t *__restrict__ sd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t q = n / streams, r = n % streams;
    int64_t t, lo;
    if (i < r * (q + 1)) {
        t = i / (q + 1);
        lo = t * (q + 1);
    } else {
        t = r + (q > 0 ? (i - r * (q + 1)) / q : 0);
        lo = r * (q + 1) + (t - r) * q;
    }
    uint64_t c = (uint64_t)(calls_excl[i] - calls_excl[lo]);
    if (streams == 1) c += calls_before;
    // three LCG steps per rand_r call; the LCG has period 2^32.  The pair leaves NORMALISED: (state of the stream at the root's
    // first draw, 0 further steps) names the same point of the stream as (seed + t, 3c) and spares every workgroup of the walk
    // kernels the 32-round jump from the seed (they compute lcg_jump(seed, pos + ...): 0 rounds for pos = 0)
    pos[i] = 0u;
    sd[i] = lcg_jump(seed + (uint32_t)t, (uint32_t)(3ull * c));
}

// step_prologue_kernel (uniq.hip) for a step whose roots come as two arrays -- the heads every K segments share (the sources of an
// evaluation batch, utils.py:93-95; u and v of the higher-order negatives, dataloader.py:265-275) and the tails (the candidates) --
// in ONE launch: table reset, status words zeroed, roots[0 .. n_heads) = heads and roots[n_heads .. n_heads + n_tails) = tails,
// narrowed as the plain prologue narrows.
__global__ void step_prologue_star_kernel(UniqTable t, int64_t cap, int64_t *zero_words, int64_t n_zero, const int64_t *heads,
                                          int64_t n_heads, const int64_t *tails, int64_t n_tails, int32_t *roots) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) uniq_reset_slot(t, i);        // cap = 0: no table (key rows)
    if (i < n_zero) zero_words[i] = 0;
    if (i < n_heads + n_tails) roots[i] = narrow_root(i < n_heads ? heads[i] : tails[i - n_heads]);
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_step_prologue_star(void *table, int64_t capacity, int64_t *zero_words, int64_t n_zero, const int64_t *heads,
                                          int64_t n_heads, const int64_t *tails, int64_t n_tails, int32_t *roots, void *stream) {
    SG_REQUIRE(!table || (capacity > 0 && (capacity & (capacity - 1)) == 0 && capacity < (1ll << 31)), SUBGACC_ERR_BADARG,
               "step_prologue_star: capacity must be a power of two below 2^31");
    if (!table) capacity = 0;
    SG_REQUIRE(n_heads >= 0 && n_tails >= 0 && n_zero >= 0, SUBGACC_ERR_BADARG,
               "step_prologue_star: negative count (n_heads = %lld, n_tails = %lld, n_zero = %lld)", (long long)n_heads,
               (long long)n_tails, (long long)n_zero);
    SG_REQUIRE(n_heads < (1ll << 30) && n_tails < (1ll << 30) && n_heads + n_tails < (1ll << 30), SUBGACC_ERR_BADARG,
               "step_prologue_star: n_heads + n_tails = %lld + %lld roots (must be below 2^30)", (long long)n_heads, (long long)n_tails);
    const int64_t n = n_heads + n_tails;
    SG_REQUIRE((n == 0 || roots) && (n_heads == 0 || heads) && (n_tails == 0 || tails) && (n_zero == 0 || zero_words),
               SUBGACC_ERR_BADARG, "step_prologue_star: null argument");
    SG_REQUIRE(n_zero < (1ll << 30), SUBGACC_ERR_BADARG, "step_prologue_star: n_zero = %lld status words (must be below 2^30)",
               (long long)n_zero);
    const int64_t span = prologue_span(capacity, n_zero, n);
    if (span == 0) return SUBGACC_OK;
    hipLaunchKernelGGL(step_prologue_star_kernel, dim3((unsigned)ceil_div(span, 256)), dim3(256), 0, (hipStream_t)stream,
                       table ? uniq_view(table, capacity) : UniqTable{nullptr, nullptr, nullptr, 0}, capacity, zero_words, n_zero,
                       heads, n_heads, tails, n_tails, roots);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

extern "C" int subgacc_key_shift(int32_t num_walks, int32_t num_steps) {
    SG_REQUIRE(num_walks > 0 && num_steps > 0, SUBGACC_ERR_BADARG, "num_walks and num_steps must be positive");
    const int shift = 32 - __builtin_clz((unsigned)num_walks);
    SG_REQUIRE((int64_t)num_steps * shift + 1 <= 64, SUBGACC_ERR_KEYWIDTH,
               "Longer width of type for hasing key needed > INT64.");
    // an all-ones key would collide with the empty marker of the unique table
    SG_REQUIRE(!((int64_t)num_steps * shift + 1 == 64 && num_walks == (1 << shift) - 1), SUBGACC_ERR_KEYWIDTH,
               "key space exhausted: num_steps*SHIFT+1 == 64 with num_walks == 2^SHIFT-1");
    return shift;
}

extern "C" size_t subgacc_rng_positions_workspace_bytes(int64_t n) {
    if (n < 0) n = 0;
    return align_up((size_t)n * 4, 256) + align_up((size_t)(n + 1) * 8, 256) + scan_workspace_bytes(n);
}

extern "C" int subgacc_rng_positions(const subgacc_walk_cfg *cfg, const void *indptr, int64_t num_nodes,
                                     const int32_t *query, int64_t n, int32_t rng_streams, uint64_t calls_before, uint32_t *rng_pos,
                                     uint32_t *rng_seed, void *workspace, size_t workspace_bytes, void *stream) {
    SG_REQUIRE(cfg && indptr && rng_pos && rng_seed && n >= 0 && num_nodes >= 0, SUBGACC_ERR_BADARG,
               "rng_positions: null argument");
    SG_REQUIRE(rng_streams >= 1, SUBGACC_ERR_BADARG, "rng_positions: rng_streams must be >= 1");
    SG_REQUIRE(rng_streams == 1 || calls_before == 0, SUBGACC_ERR_BADARG,
               "rng_positions: calls_before only makes sense for a single stream");
    if (n == 0) return SUBGACC_OK;
    SG_REQUIRE(query, SUBGACC_ERR_BADARG, "rng_positions: null query");
    SG_REQUIRE(workspace && workspace_bytes >= subgacc_rng_positions_workspace_bytes(n), SUBGACC_ERR_WORKSPACE,
               "rng_positions: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int32_t *calls = (int32_t *)ws;
    ws += align_up((size_t)n * 4, 256);
    int64_t *excl = (int64_t *)ws;
    ws += align_up((size_t)(n + 1) * 8, 256);
    const unsigned grid = (unsigned)ceil_div(n, 256);
    if (cfg->indptr64)
        hipLaunchKernelGGL(rng_calls_kernel<true>, dim3(grid), dim3(256), 0, s, indptr, query, n, num_nodes, cfg->num_walks,
                           cfg->num_steps, cfg->first_hop_wo, cfg->cap_root_degree, calls);
    else
        hipLaunchKernelGGL(rng_calls_kernel<false>, dim3(grid), dim3(256), 0, s, indptr, query, n, num_nodes, cfg->num_walks,
                           cfg->num_steps, cfg->first_hop_wo, cfg->cap_root_degree, calls);
    SG_LAUNCH_CHECK();
    int rc = exclusive_scan_i32(calls, n, excl, ws, workspace_bytes - (size_t)(ws - (char *)workspace), s);
    if (rc != SUBGACC_OK) return rc;
    hipLaunchKernelGGL(rng_positions_kernel, dim3(grid), dim3(256), 0, s, (const int64_t *)excl, n, rng_streams,
                       calls_before, cfg->seed, rng_pos, rng_seed);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

template <bool IDX64>
__global__ void hop_records_kernel(const void *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t num_nodes,
                                   int64_t nnz, RecFmt f, unsigned long long *__restrict__ recs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int32_t v = indices[e];
    int64_t beg = 0, deg = 0;
    if ((uint64_t)(int64_t)v < (uint64_t)num_nodes) load_row<IDX64>(indptr, v, beg, deg);
    const int deg_bits = 64 - f.id_bits - f.beg_bits;
    const unsigned long long dmask = (1ull << deg_bits) - 1ull;
    const unsigned long long dv = (unsigned long long)deg >= dmask ? dmask : (unsigned long long)deg;   // all ones = escape
    recs[e] = ((unsigned long long)(uint32_t)v << (64 - f.id_bits)) | ((unsigned long long)beg << deg_bits) | dv;
}

// 16-byte form for graphs with int64 row offsets: {neighbour id : 32 | its degree : 32 (saturated), its row begin : 64}
template <bool IDX64>
__global__ void hop_records16_kernel(const void *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t num_nodes,
                                     int64_t nnz, ulonglong2 *__restrict__ recs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int32_t v = indices[e];
    int64_t beg = 0, deg = 0;
    if ((uint64_t)(int64_t)v < (uint64_t)num_nodes) load_row<IDX64>(indptr, v, beg, deg);
    recs[e] = make_ulonglong2(((unsigned long long)(deg > 0xFFFFFFFFll ? 0xFFFFFFFFull : (unsigned long long)deg) << 32) | (uint32_t)v,
                              (unsigned long long)beg);
}

extern "C" int subgacc_hop_records_format(int64_t num_nodes, int64_t nnz, int32_t *id_bits, int32_t *beg_bits) {
    SG_REQUIRE(num_nodes >= 0 && nnz >= 0 && id_bits && beg_bits, SUBGACC_ERR_BADARG, "hop_records_format: bad arguments");
    int ib = 1, bb = 1;
    while (ib < 32 && ((int64_t)1 << ib) < num_nodes) ++ib;
    while (bb < 40 && ((int64_t)1 << bb) <= nnz) ++bb;
    *id_bits = ib, *beg_bits = bb;
    const int deg_bits = 64 - ib - bb;
    SG_REQUIRE(deg_bits >= 8, SUBGACC_ERR_BADARG, "hop_records_format: only %d bits left for the degree", deg_bits);
    return deg_bits;
}

extern "C" int subgacc_hop_records_build(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes,
                                         int64_t nnz, int32_t id_bits, int32_t beg_bits, uint64_t *recs, void *stream) {
    SG_REQUIRE(indptr && num_nodes >= 0 && nnz >= 0, SUBGACC_ERR_BADARG, "hop_records_build: bad arguments");
    if (id_bits == 0 && beg_bits == 0) {     // the 16-byte form (2 uint64 per entry)
        if (nnz == 0) return SUBGACC_OK;
        SG_REQUIRE(indices && recs, SUBGACC_ERR_BADARG, "hop_records_build: null argument");
        const int64_t blocks16 = ceil_div(nnz, 256);
        SG_REQUIRE(blocks16 < (1ll << 31), SUBGACC_ERR_BADARG, "hop_records_build: graph too large for one launch");
        if (indptr64)
            hipLaunchKernelGGL(hop_records16_kernel<true>, dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, indptr,
                               indices, num_nodes, nnz, (ulonglong2 *)recs);
        else
            hipLaunchKernelGGL(hop_records16_kernel<false>, dim3((unsigned)blocks16), dim3(256), 0, (hipStream_t)stream, indptr,
                               indices, num_nodes, nnz, (ulonglong2 *)recs);
        SG_LAUNCH_CHECK();
        return SUBGACC_OK;
    }
    SG_REQUIRE(id_bits >= 1 && beg_bits >= 1 && id_bits + beg_bits <= 56, SUBGACC_ERR_BADARG, "hop_records_build: bad field widths");
    SG_REQUIRE(num_nodes <= ((int64_t)1 << id_bits) && nnz < ((int64_t)1 << beg_bits), SUBGACC_ERR_BADARG,
               "hop_records_build: the graph does not fit id_bits = %d / beg_bits = %d", id_bits, beg_bits);
    if (nnz == 0) return SUBGACC_OK;
    SG_REQUIRE(indices && recs, SUBGACC_ERR_BADARG, "hop_records_build: null argument");
    const RecFmt f{id_bits, beg_bits};
    const int64_t blocks = ceil_div(nnz, 256);
    SG_REQUIRE(blocks < (1ll << 31), SUBGACC_ERR_BADARG, "hop_records_build: graph too large for one launch");
    if (indptr64)
        hipLaunchKernelGGL(hop_records_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, indptr, indices,
                           num_nodes, nnz, f, (unsigned long long *)recs);
    else
        hipLaunchKernelGGL(hop_records_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, indptr, indices,
                           num_nodes, nnz, f, (unsigned long long *)recs);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}
