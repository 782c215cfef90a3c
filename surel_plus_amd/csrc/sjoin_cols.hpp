// sjoin_cols.hpp -- where the count and index kernels take a member's column from (internal): the member's SFptr itself for a packed
// store (TableColumns: sjoin_counts_attn_kernel, sjoin_forms.hip) or the rank of its LP key in the sorted key list of a step
// (KeyColumns: sjoin_key_counts_attn_kernel and sjoin_key_index_kernel, sjoin_keys.hip), and a float's order-preserving integer image (sjoin_attn.hpp).
#pragma once
#include "sjoin.hpp"

namespace subgacc {

// The column of `key`: its rank in the sorted LDS array keys[0, n), by halving (the trip count depends on n alone), or -1
__device__ __forceinline__ int32_t kc_column(const uint32_t *keys, int n, uint32_t key) {
    int b = 0;
    const int n0 = n;
    while (n > 1) {
        const int h = n >> 1;
        b = keys[b + h] <= key ? b + h : b;
        n -= h;
    }
    return (n0 > 0 && keys[b] == key) ? b + 1 : -1;
}

// A column policy: open(rows) before anything else of the kernel (what it reads is on its way with S's first members), stage(lds)
// where the kernel fills LDS, column(word, col) -> is the payload word valid, with its column in col; lengths() at the end.

// A packed SFptr store: the payload word is the column, valid inside the table.  Nothing is staged, nothing but the rows is written.
struct TableColumns {
    static constexpr bool kStaged = false;
    int rows;
    __device__ __forceinline__ void open(int rows_) { rows = rows_; }
    __device__ __forceinline__ void stage(uint32_t *) {}
    __device__ __forceinline__ bool column(int32_t v, int32_t &col) const {
        col = v;
        return (uint32_t)v < (uint32_t)rows;
    }
    __device__ __forceinline__ void lengths(int64_t, int, int64_t, int) const {}
};

// The key rows of a step: the payload word is a 32-bit LP key, its column the key's rank among the step's sorted distinct keys
// (subgacc_keyrows_columns), -1 and invalid for a key that is not in the list.  kStaged: the keys go to LDS first -- a kernel maps the
// members it staged only after a barrier behind stage().  out_len (NULL = not wanted): the lengths of a pair's two segments.
// sjoin_key_index_kernel builds its own from __restrict__ arguments: a struct's members cannot promise that, and without it the
// kernel needs 10 VGPRs more.
struct KeyColumns {
    static constexpr bool kStaged = true;
    const uint32_t *ukeys;                      // the step's sorted distinct keys, and their number on the device
    const int64_t *n_keys;
    int32_t *out_len;
    const uint32_t *keys = nullptr;             // (set by stage: the keys in LDS)
    int nk = 0;
    __device__ __forceinline__ void open(int rows) {
        const int64_t c64 = *n_keys;
        nk = (int)(c64 < 0 ? 0 : (c64 > rows - 1 ? rows - 1 : c64));      // never more keys than columns
    }
    // rows - 1 words of LDS at `lds`, filled by a workgroup of kPairThreads lanes
    __device__ __forceinline__ void stage(uint32_t *lds) {
        for (int x = threadIdx.x; x < nk; x += kPairThreads) lds[x] = ukeys[x];
        keys = lds;
    }
    __device__ __forceinline__ bool column(int32_t key, int32_t &col) const {
        col = kc_column(keys, nk, (uint32_t)key);
        return col >= 0;
    }
    __device__ __forceinline__ void lengths(int64_t jS, int ns, int64_t jT, int nt) const {
        if (out_len && threadIdx.x == 0) out_len[jS] = ns, out_len[jT] = nt;
    }
};

// a member's column from its payload word; an invalid one (outside the table, a key not in the list) raises flags[3] |= 2 and is read
// as column 0, never out of bounds
template <class Cols>
__device__ __forceinline__ int32_t member_column(const Cols &cols, int32_t word, int32_t *flags) {
    int32_t v;
    if (!cols.column(word, v)) atomicOr(&flags[3], 2), v = 0;
    return v;
}

__device__ __forceinline__ int32_t ord_of(float f) {     // a float as an int of the same order (max by integer atomics: exact)
    const int32_t b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float float_of(int32_t o) { return __int_as_float(o >= 0 ? o : o ^ 0x7FFFFFFF); }

// What every entry point over the key rows of a step refuses alike about its descriptor, in this order: subgacc_sjoin_key_counts, the
// attentional pair and subgacc_sjoin_key_index (sjoin_keys.hip; rows_form: the index form, which has always looked at its form before
// the options), subgacc_sjoin_key_mean (sjoin_mean.hip) and subgacc_sjoin_key_attn (sjoin_key_attn.hip)
static int key_join_check(const char *name, const subgacc_join_desc *d, RowLayout &layout, bool rows_form = false) {
    if (int rc = decode_desc(name, d, true, layout)) return rc;
    SG_REQUIRE(!rows_form || d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG,
               "%s: writes the index pairs of the row form (form ROWS), not form %d", name, (int)d->form);
    SG_REQUIRE(d->options == 0, SUBGACC_ERR_BADARG, "%s: takes no option (options = %d)", name, (int)d->options);
    SG_REQUIRE(d->payload_kind == SUBGACC_JOIN_KEY32, SUBGACC_ERR_BADARG,
               "%s: joins rows of 32-bit LP keys (KEY32), not payload kind %d", name, (int)d->payload_kind);
    SG_REQUIRE(layout == RowLayout::Strided, SUBGACC_ERR_BADARG,
               "%s: joins the strided key rows of a step (row_len and row_stride set, row_off NULL), not packed or headed rows", name);
    SG_REQUIRE(d->table_rows >= 2 && d->table_rows < (1ll << 31), SUBGACC_ERR_BADARG,
               "%s: table_rows = %lld (the absent column and at least one LP row: >= 2)", name, (long long)d->table_rows);
    return SUBGACC_OK;
}

}  // namespace subgacc
