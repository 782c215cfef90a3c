// row_sort.hpp -- the pieces of the two-level bucket sort that puts a sampled set in id order inside the workgroup's LDS: the table
// form's epilogue of walk_rows_kernel (walk_rows.hip), its key-row epilogue, and the fused epilogue of walk_sets_kernel<SPG>
// (walk.hip).  Free functions that take what they need by value: each is compiled on its own before it is inlined, and one that
// reached its operands through a pointer to the kernel's state came out as different instructions (walk_rows.hip's header).
// red[] is the workgroup's 16 reduction words: [4 ..) the waves' largest counts, [12 ..) the waves' totals.
#pragma once
#include "common.hpp"
#include "waveops.hpp"

namespace subgacc {

// level 1's geometry: B <= min(T/4, NT) buckets of 2^bshift ids over the set's ns ids in [mn, mx]
template <int T, int NT>
__device__ __forceinline__ void rows_bucket_geometry(int32_t ns, int32_t mn, int32_t mx, int &B, int &bshift) {
    int logb = 0;
    while ((1 << logb) < ns && (2 << logb) <= T / 4 && (2 << logb) <= NT) ++logb;
    B = 1 << logb;
    const uint32_t range = (uint32_t)(mx - mn) + 1u;
    const int Ls = (range <= 1u) ? 0 : (32 - __builtin_clz(range - 1u));
    bshift = Ls > logb ? Ls - logb : 0;      // (id - mn) < 2^Ls, and ns <= range => logb <= Ls
}
// the same with T and NT at run time (walk_sets_kernel).  An overload with its own loop: as the template forwarding to this one every
// walk_rows_kernel came out as different instructions (tools/kernel_digest.py)
__device__ __forceinline__ void rows_bucket_geometry(int T, int NT, int32_t ns, int32_t mn, int32_t mx, int &B, int &bshift) {
    int logb = 0;
    while ((1 << logb) < ns && (2 << logb) <= T / 4 && (2 << logb) <= NT) ++logb;
    B = 1 << logb;
    const uint32_t range = (uint32_t)(mx - mn) + 1u;
    const int Ls = (range <= 1u) ? 0 : (32 - __builtin_clz(range - 1u));
    bshift = Ls > logb ? Ls - logb : 0;
}

// level 1 of the key rows' sort: exclusive scan over the B <= NT buckets, one bucket per lane: wave scan, then (two waves) the
// wave totals through LDS -> the largest count
// (a wave's base = the totals of the waves in front of it: at most NT / 64 - 1 of them, spelled out -- as a loop over
//  tid / 64 the compiler vectorised it into 16-byte reads with a scalar tail, ~60 instructions for one addition)
template <int NT>
__device__ __forceinline__ int32_t rows_level1_scan(int32_t *start, int32_t *red, int B, int tid) {
    const int32_t c = tid < B ? start[tid] : 0;
    const int32_t inc = wave_scan_add_i32_incl(c);     // inclusive scan over the wave
    const int32_t mc = wave_red_max_i32(c);
    int32_t base = 0, maxc = mc;
    if (NT > kWave) {
        if ((tid & (kWave - 1)) == kWave - 1) red[12 + tid / kWave] = inc, red[4 + tid / kWave] = mc;
        __syncthreads();
#pragma unroll
        for (int w2 = 0; w2 < NT / kWave - 1; ++w2) base += w2 < tid / kWave ? red[12 + w2] : 0;
        maxc = red[4];
#pragma unroll
        for (int w2 = 1; w2 < NT / kWave; ++w2) maxc = max(maxc, red[4 + w2]);
    }
    const int32_t excl = base + inc - c;
    if (tid < B) start[tid] = excl;
    if (tid == B - 1) start[B] = excl + c;
    return maxc;
}

// Where a member goes at level 2: its level-1 bucket b1 (from lo1 on, kb / fine members) is cut into kb parts of equal id width;
// ido = id - min, off = the member's offset in the bucket's id window, sub = its part
struct RowsPart {
    uint32_t lo1, kb, off, sub;
};
__device__ __forceinline__ RowsPart rows_part(const int32_t *start, uint32_t ido, uint32_t b1, int bshift, uint32_t fine) {
    RowsPart p;
    p.lo1 = (uint32_t)start[b1];
    p.kb = ((uint32_t)start[b1 + 1] - p.lo1) * fine;
    p.off = ido - (b1 << bshift);                                                  // < 2^bshift
    p.sub = bshift ? __umulhi(p.off << (32 - bshift), p.kb) : 0u;                 // floor(off * kb / 2^bshift) < kb
    return p;
}

// one more member in the 16-bit counter idx (two per word) -> its arrival order
__device__ __forceinline__ uint32_t rows_count16(uint32_t *cnt2, uint32_t idx) {
    const uint32_t sh = (idx & 1u) * 16u;
    return (atomicAdd(&cnt2[idx >> 1], 1u << sh) >> sh) & 0xFFFFu;
}

// level 2: exclusive scan of the 16-bit counters (two per word, W2 <= CW * NT words) in place -- the offsets stay below 2^16 -- with CW
// consecutive words per lane; every lane of the workgroup calls it, between two barriers of the caller's
template <int NT, int CW>
__device__ __forceinline__ void rows_level2_scan(uint32_t *cnt2, int W2, int32_t *red, int tid) {
    uint32_t w[CW];
    int32_t s2 = 0;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int x = tid * CW + c;
        w[c] = x < W2 ? cnt2[x] : 0u;
        s2 += (int32_t)((w[c] & 0xFFFFu) + (w[c] >> 16));
    }
    const int32_t inc = wave_scan_add_i32_incl(s2);
    if ((tid & (kWave - 1)) == kWave - 1) red[12 + tid / kWave] = inc;
    __syncthreads();
    int32_t run = inc - s2;
#pragma unroll
    for (int w2 = 0; w2 < NT / kWave - 1; ++w2) run += w2 < tid / kWave ? red[12 + w2] : 0;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int x = tid * CW + c;
        const uint32_t lo16 = (uint32_t)run;
        run += (int32_t)(w[c] & 0xFFFFu);
        const uint32_t hi16 = (uint32_t)run;
        run += (int32_t)(w[c] >> 16);
        if (x < W2) cnt2[x] = lo16 | (hi16 << 16);
    }
}

}  // namespace subgacc
