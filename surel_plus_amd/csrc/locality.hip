// locality.hip -- one round of the deterministic label propagation behind sampler.locality_order (gfx950).
//
// The walk kernel takes the rows of a batch in the order of a work list (subgacc_worklist_by_root / _by_rank): roots that stand
// next to each other on the list are walked at the same time on the same XCD and share its L2.  Ascending root id only helps where
// ids carry locality (communities of consecutive ids); a rank that puts the members of a community next to each other gives the
// same gain to a graph whose ids carry none.  This pass builds the communities: labels start as the node's own id, and a node
// that updates in round t takes the most frequent label among (a sample of) its neighbours' labels and its own.  The host sorts
// the nodes by (label, id) once (sampler.locality_order): that is the rank.
//
// The rule, fixed so that a NumPy restatement reproduces it bit for bit (tests/test_locality_cpu.py):
//   - node v updates in round t iff (mix32(v) & 1) == (t & 1) (half of the nodes per round: a fully synchronous round lets two
//     neighbours swap labels forever); every other node copies its label;
//   - an updating node with deg > 0 reads the labels of k = min(deg, cap) neighbours: all of them if deg <= cap, otherwise the ones
//     at positions j*deg/cap (64-bit integer division), j < cap; its own label counts once more; the new label is the most
//     frequent of these, the smallest label among equally frequent ones;
//   - a node without neighbours keeps its label.
// mix32 is the 32-bit hash of include/subgacc.h.
//
// One wave per node (cap <= 64: one candidate label per lane).  Lane j gathers candidate j, counts how many of the k candidates
// equal its own by k v_readlane broadcasts (scalar registers, no LDS), and two DPP reductions pick the mode.  Nodes that do not
// update this round cost their wave one load and one store.
#include "common.hpp"
#include "waveops.hpp"

namespace subgacc {

constexpr int kLocThreads = 256;                    // 4 waves, one node each at a time
constexpr int kLocMaxBlocks = 256 * 8;              // grid-stride beyond 8 blocks per CU

__device__ __forceinline__ uint32_t loc_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

template <bool I64>
__global__ __launch_bounds__(kLocThreads) void locality_round_kernel(const void *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                     int32_t num_nodes, const int32_t *__restrict__ lin,
                                                                     int32_t *__restrict__ lout, int32_t round, int32_t cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * (kLocThreads / kWave);
    const int32_t first = __builtin_amdgcn_readfirstlane((int32_t)blockIdx.x * (kLocThreads / kWave) + (int32_t)(threadIdx.x / kWave));
    for (int64_t vv = first; vv < num_nodes; vv += waves) {
        const int32_t v = (int32_t)vv;
        const int32_t own = lin[v];
        int64_t beg = 0, deg = 0;
        const bool upd = (int32_t)(loc_mix32((uint32_t)v) & 1u) == (round & 1);
        if (upd) {
            if (I64) {
                const int64_t *ip = (const int64_t *)indptr;
                beg = ip[v], deg = ip[v + 1] - beg;
            } else {
                const int32_t *ip = (const int32_t *)indptr;
                beg = ip[v], deg = (int64_t)ip[v + 1] - beg;
            }
        }
        if (!upd || deg <= 0) {
            if (lane == 0) lout[v] = own;
            continue;
        }
        const int32_t k = deg <= cap ? (int32_t)deg : cap;
        int32_t lab = -1;
        if (lane < k) {
            const int64_t pos = deg <= cap ? (int64_t)lane : (int64_t)lane * deg / cap;
            const int32_t u = indices[beg + pos];
            lab = (uint32_t)u < (uint32_t)num_nodes ? lin[u] : -1;        // (a neighbour outside the graph contributes nothing)
        }
        int32_t cnt = lab == own ? 1 : 0;
        for (int32_t i = 0; i < k; ++i) cnt += __builtin_amdgcn_readlane(lab, i) == lab ? 1 : 0;
        const bool cand = lab >= 0;
        const int32_t own_cnt = 1 + wave_red_add_i32(cand && lab == own ? 1 : 0);
        const int32_t best = max(wave_red_max_i32(cand ? cnt : 0), own_cnt);
        const int32_t pick = wave_red_min_i32(cand && cnt == best ? lab : INT32_MAX);
        if (lane == 0) lout[v] = own_cnt == best ? min(pick, own) : pick;
    }
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_locality_round(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes,
                                      const int32_t *labels_in, int32_t *labels_out, int32_t round, int32_t cap, void *stream) {
    SG_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31) && round >= 0 && cap >= 1 && cap <= kWave, SUBGACC_ERR_BADARG,
               "locality_round: bad arguments (0 <= num_nodes < 2^31, round >= 0, 1 <= cap <= 64)");
    SG_REQUIRE(indptr && indices && labels_in && labels_out && labels_in != labels_out, SUBGACC_ERR_BADARG,
               "locality_round: null argument (or labels_in == labels_out)");
    if (num_nodes == 0) return SUBGACC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t want = ceil_div(num_nodes, kLocThreads / kWave);
    const int nblk = (int)(want < kLocMaxBlocks ? want : kLocMaxBlocks);
    if (indptr64)
        hipLaunchKernelGGL(locality_round_kernel<true>, dim3(nblk), dim3(kLocThreads), 0, s, indptr, indices, (int32_t)num_nodes,
                           labels_in, labels_out, round, cap);
    else
        hipLaunchKernelGGL(locality_round_kernel<false>, dim3(nblk), dim3(kLocThreads), 0, s, indptr, indices, (int32_t)num_nodes,
                           labels_in, labels_out, round, cap);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}
