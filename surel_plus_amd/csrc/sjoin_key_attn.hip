// sjoin_key_attn.hip -- the LP encoder's attentional first stage fused into the attentional count join over the key rows of an
// on-demand step (gfx950): subgacc_sjoin_key_attn, include/subgacc_attn.h.
//
// sjoin_key_counts_attn_kernel<false> (sjoin_keys.hip) leaves a pair's two segments as dense softmax-weighted count rows
// W[j, 0 .. T) in global memory, and the stage behind it is the GEMM W @ E with E = embed(table) [T, H].  W is the largest object of
// that step and almost all zeros.  sjoin_key_attn_kernel has that kernel's front -- the same text: counts_attn_body<false,
// KeyColumns> of sjoin_attn.hpp, up to and including the per-column chains that leave accf[blk*rows + r] = sum / den in LDS -- and,
// where that body stores its two rows, multiplies them by E while they stand in LDS (RowsTimesE below, the body's Tail):
//   a wave takes one item = (segment of the pair, 64 features), lane = feature, and walks the columns 0 .. c as the back end of
//   sjoin_key_mean_kernel (sjoin_mean.hip) walks its histograms: 64 columns at a time, one LDS read per lane, a ballot of the words
//   whose bits are not zero, a scalar loop over the set bits in ascending order; per set bit the weight comes from LDS (one address
//   for the wave: a broadcast) and the 64 features of E's row as one coalesced 256-byte load; kBatch set bits' loads leave before
//   their adds; a column whose word of W is zero bits -- every column no member of the segment shows -- is passed over, and its
//   row of E never read;
//   the 2 * ceil(H / 64) items are dealt to the workgroup's four waves.
// The walk is written out here, not shared with sjoin_mean.hip: lifted into a header that both call, it compiled
// sjoin_key_mean_kernel to other instructions than the parent's (the same registers, two shifts and the operands of three adds
// moved), and that kernel keeps its text.  The weight is a float here and an int32 count there; there is no division
// here.
// One summation chain per (segment, feature), in ascending column order, a separate multiply and add (the library is built with
// -ffp-contract=off; no fused multiply-add is written here): the documented result, so the same bits for every schedule.  m_j,
// den_j and out_len are written by the body's own text, after the tail.  LDS is the unfused forward's: W lives there already and E is
// not staged.
#include "sjoin_attn.hpp"
#include "../../include/subgacc_attn.h"

namespace subgacc {

constexpr int kAttnMaxWidth = 1024;
constexpr int kBatch = 4;          // set bits whose loads of E are asked for together

// counts_attn_body's Tail: the pair's two rows of W in LDS times E, out_a in the place of out_w
struct RowsTimesE {
    static constexpr bool kFused = true;
    const float *e;         // [table_rows, H]
    int32_t H;
    float *out_a;           // [S, H]
    __device__ __forceinline__ void operator()(const float *accf, int rows, const KeyColumns &cols, int64_t jS, int64_t jT) const {
        const int tid = threadIdx.x;
        const int ncol = cols.nk + 1;                       // a column past the keys holds no weight (kc_column answers 1 .. c)
        const int lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
        const int chunks = (H + kWave - 1) / kWave;
        for (int item = wave; item < 2 * chunks; item += kPairThreads / kWave) {
            const bool isT = item & 1;
            const int32_t *row = (const int32_t *)accf + (isT ? rows : 0);
            const int h = (item >> 1) * kWave + lane;
            const bool live = h < H;
            const float *eh = e + (live ? h : 0);
            float acc = 0.0f;
            for (int x0 = 0; x0 < ncol; x0 += kWave) {
                const int x = x0 + lane;
                const int32_t mine = x < ncol ? row[x] : 0;
                unsigned long long mask = __ballot(mine != 0);
                while (mask) {
                    int32_t wb[kBatch];
                    float ev[kBatch];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) {      // the loads of up to kBatch set bits, in ascending column order
                        wb[u] = 0, ev[u] = 0.0f;
                        if (mask) {
                            const int xb = x0 + __builtin_ctzll(mask);
                            mask &= mask - 1;
                            wb[u] = row[xb];                // one address for the wave: an LDS broadcast
                            if (live) ev[u] = eh[(int64_t)xb * H];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kBatch; ++u)        // the chain: multiply, then add
                        if (wb[u]) {
                            const float p = __int_as_float(wb[u]) * ev[u];
                            acc = acc + p;
                        }
                }
            }
            if (live) __builtin_nontemporal_store(acc, out_a + (isT ? jT : jS) * (int64_t)H + h);
        }
    }
};

__global__ __launch_bounds__(kPairThreads) void sjoin_key_attn_kernel(const JoinArgs a, int64_t pb, int32_t dcap, const CountsAttnArgs c,
                                                                      const KeyColumns cols, const float *__restrict__ e, int32_t H,
                                                                      float *__restrict__ out_a) {
    counts_attn_body<false>(a, pb, dcap, c, cols, RowsTimesE{e, H, out_a});
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_sjoin_key_attn(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g,
                                      const float *e, int32_t width, float *out_a, float *out_max, float *out_den, int32_t *out_len,
                                      void *stream) {
    const char *name = "sjoin_key_attn";
    RowLayout layout;
    if (int rc = key_join_check(name, d, layout)) return rc;       // every refusal of subgacc_sjoin_key_counts, in its order
    SG_REQUIRE(ukeys && n_keys && g && e && out_a, SUBGACC_ERR_BADARG,
               "%s: ukeys, n_keys, g, e and out_a are required (a NULL one given)", name);
    SG_REQUIRE((out_max == nullptr) == (out_den == nullptr), SUBGACC_ERR_BADARG, "%s: out_max and out_den go together (one is NULL)", name);
    SG_REQUIRE(width >= 1 && width <= kAttnMaxWidth, SUBGACC_ERR_BADARG, "%s: width = %d (the features of a row of e: 1 .. %d)", name,
               (int)width, kAttnMaxWidth);
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    int32_t dcap;
    size_t lds;
    if (int rc = counts_attn_fit(name, a, a.table_rows - 1, false, out_max != nullptr,
                                 "%s: table_rows = %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the "
                                 "row form",
                                 "%s: table_rows = %lld columns and rows of %d members: the backward needs %zu B of LDS; use a smaller "
                                 "table_rows or the row form", dcap, lds))
        return rc;
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    const CountsAttnArgs c{g, nullptr, out_max, out_den, nullptr, nullptr, nullptr, nullptr, nullptr};
    return launch(sjoin_key_attn_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, d->pair_block, dcap, c,
                  KeyColumns{(const uint32_t *)ukeys, n_keys, out_len}, e, width, out_a);
}
