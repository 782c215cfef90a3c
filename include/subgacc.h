/*
 * subgacc.h -- C ABI of the MI355X-native SubGAcc hot path (libsubgacc_hip.so, gfx950).
 *
 * This is the drop-in boundary for the SUREL+ path
 *     sample (random-walk node sets + landing-probability counts)  ->  SpG  ->  SpJoin.
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * tree, Graph-COM/SUREL_Plus).  The reference binds its C half through a CPython module
 * (`subg_acc`, subg_acc/subg_acc.c:1036-1059) and runs SpJoin in SciPy (train.py:13-111); the host
 * mirror of both lives in surel_plus_amd/ and is a thin ctypes layer over the functions below.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / numpy / HIP types in any signature.
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and nothing
 *     synchronises unless the function says so.  No allocation happens inside: scratch comes
 *     from the caller (`*_workspace_bytes`), so calls are graph-capturable.
 *   - return value: SUBGACC_OK or a negative subgacc_status; subgacc_last_error() gives the text
 *     (thread local).
 *   - node ids are int32 (the reference is int32-only, subg_acc.c:663-676); CSR row offsets may be
 *     int32 or int64 (`indptr64`), SpG row offsets are always int64.
 */
#ifndef SUBGACC_H
#define SUBGACC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGACC_ABI_VERSION 7

typedef enum subgacc_status {
    SUBGACC_OK = 0,
    SUBGACC_ERR_BADARG = -1,    /* TypeError("Input parsing error.") territory, subg_acc.c:658 */
    SUBGACC_ERR_WORKSPACE = -2, /* caller's scratch too small (the reference's MemoryError paths) */
    SUBGACC_ERR_KEYWIDTH = -3,  /* m*SHIFT+1 > 64: AssertionError, subg_acc.c:905-915 */
    SUBGACC_ERR_CAPACITY = -4,  /* unique-row table full: retry with a larger one */
    SUBGACC_ERR_HIP = -5,       /* a HIP runtime call failed */
    SUBGACC_ERR_LDS = -6,       /* M*m+1 too large for the per-root LDS tables */
    SUBGACC_ERR_NODEVICE = -7   /* no gfx950 device visible */
} subgacc_status;

enum { SUBGACC_RNG_RAND_R = 0, /* glibc rand_r stream, bit-exact with the reference at nthread=1 */
       SUBGACC_RNG_PHILOX = 1  /* Philox2x32-10, key = seed, counter = (root id, walk | draw block | stream tag): schedule independent */ };
enum { SUBGACC_ORDER_WALK_MAJOR = 0, /* set_sampler's first-visit order, subg_acc.c:785-832 */
       SUBGACC_ORDER_STEP_MAJOR = 1  /* rpe_encoder's first-visit order, subg_acc.c:263-278 */ };

int subgacc_abi_version(void);
const char *subgacc_last_error(void);
/* number of visible HIP devices whose arch is gfx950 (0 => every compute call fails loudly) */
int subgacc_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Sampler: walks + per-root node-set dedup + landing-probability counts.
 * Replaces the hot loop of set_sampler (subg_acc.c:742-846), random_walk (:144-180),
 * random_walk_wo (:183-247) and rpe_encoder (:249-314).
 * ------------------------------------------------------------------------------------------- */
typedef struct subgacc_walk_cfg {
    int32_t num_walks;       /* M                                                             */
    int32_t num_steps;       /* m = hops per walk (gset_sampler's num_steps; CLI --num_steps-1) */
    int32_t bucket;          /* cap on the set size; <=0 => M*m+1 (subg_acc.c:680)              */
    int32_t rng_mode;        /* SUBGACC_RNG_*                                                   */
    uint32_t seed;
    int32_t first_hop_wo;    /* 1: first hop without replacement (set_sampler, random_walk_wo)  */
    int32_t order;           /* SUBGACC_ORDER_*                                                 */
    int32_t cap_root_degree; /* 1: clamp the root degree to 1e6 (NEBMAX, subg_acc.c:750)        */
    int32_t indptr64;        /* CSR row offsets are int64 (else int32)                          */
    int32_t emit_walks;      /* 1: also write raw walks int32[n, M*(m+1)] (walk_sampler)        */
    /* ABI 3: optional packed hop records of the graph (subgacc_hop_records_build), NULL = none.  The fused-row kernel
     * then makes ONE dependent 8-byte read per hop (neighbour id + its row begin + its degree) instead of a neighbour
     * read followed by a row-pointer read; results are identical.  rec_id_bits / rec_beg_bits as given to the build;
     * both 0 = the 16-byte form.  The 8-byte form goes with int32 row offsets, the 16-byte form with int64 (a mismatch is
     * ignored: the plain CSR is walked). */
    const void *hop_records;
    int32_t rec_id_bits, rec_beg_bits;
    /* ABI 4: RAND_R on a graph with dead ends -- the stream position (LCG steps from the stream's seed) of every WALK,
     * uint32 [n * num_walks] for the n roots of the call, from subgacc_rng_replay; NULL = positions follow from the
     * degrees (subgacc_rng_positions), the symmetrised graphs of the reference's loader. */
    const uint32_t *walk_pos;
    /* ABI 6: words between the rows of two consecutive roots in the strided outputs (set_ids / set_keys / row_ids / row_slot); 0 =
     * the row capacity itself (bucket, or M*m+1).  A multiple of 32 puts every row on a 128-byte line: the join reads and the walk
     * kernels write whole lines.  Whoever reads the rows afterwards takes the same number as its `stride` / `row_stride`. */
    int32_t row_pitch;
} subgacc_walk_cfg;

/* Hop records: rec[e] = [indices[e] : id_bits | indptr[indices[e]] : beg_bits | degree(indices[e]) : rest], one uint64 per
 * CSR entry (8*nnz bytes).  subgacc_hop_records_format picks the field widths for a graph and returns the bits left for
 * the degree (a degree that does not fit is stored as all ones: the kernel reads the row pointers for that node), or
 * SUBGACC_ERR_BADARG when fewer than 8 are left (records are not worth building then).
 * id_bits = beg_bits = 0 builds the 16-byte form {id : 32 | degree : 32, row begin : 64} (recs: 2 uint64 per entry, 16*nnz
 * bytes) -- what a graph with int64 row offsets takes. */
int subgacc_hop_records_format(int64_t num_nodes, int64_t nnz, int32_t *id_bits, int32_t *beg_bits);
int subgacc_hop_records_build(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes, int64_t nnz,
                              int32_t id_bits, int32_t beg_bits, uint64_t *recs, void *stream);

/* LP rows are carried as one packed 64-bit key: count of step j in bits [(m-j)*SHIFT, +SHIFT),
 * SHIFT = 32-clz(M), plus bit m*SHIFT (LEAD) on the root row -- the reference's `bithash`
 * (subg_acc.c:900-955).  Returns SHIFT, or SUBGACC_ERR_KEYWIDTH. */
int subgacc_key_shift(int32_t num_walks, int32_t num_steps);

/* RAND_R mode only: per-root position in the sequential rand_r stream.  The reference consumes
 * calls(r) = (deg>M ? M : 0) + M*(m-1) draws per non-isolated root (first_hop_wo) or M*m
 * (plain walks), in root order; stream t of `rng_streams` owns libgomp's static chunk t of the n
 * roots and starts from seed+t (subg_acc.c:157-158,191-192; one stream for set_sampler :731-732).
 * Writes the pair (rng_seed[i], rng_pos[i]) = (an LCG state, LCG steps to take from it) that names root i's first draw; the
 * walk entry points only ever use it as lcg_jump(rng_seed[i], rng_pos[i] + ...).  It leaves NORMALISED -- rng_seed[i] = the
 * state of stream t after the draws before root i, rng_pos[i] = 0 -- so that no workgroup has to make the jump again.
 * `calls_before` = draws consumed before query[0] (for sharded / chunked callers). */
size_t subgacc_rng_positions_workspace_bytes(int64_t n);
int subgacc_rng_positions(const subgacc_walk_cfg *cfg, const void *indptr, int64_t num_nodes, const int32_t *query, int64_t n,
                          int32_t rng_streams, uint64_t calls_before, uint32_t *rng_pos, uint32_t *rng_seed,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The same positions for a graph WITH dead ends (a reached node without out-edges draws nothing in the reference and the
 * walk stays there, subg_acc.c:804-808, :168-172, :236-240: the position of every later draw then depends on how the earlier
 * walks ended).  One wavefront per stream replays it -- 64 walks at a time, right up to the first walk that ended early --
 * and writes rng_pos / rng_seed as above plus walk_pos [n * num_walks], which the walk entry points take through
 * cfg->walk_pos (they then run their general kernel).  Costs one dependent read per hop per walk of the sequential stream:
 * a fall-back for inputs the reference accepts, taken by the host mirror when a walk kernel reports flags[0] & 1. */
int subgacc_rng_replay(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                       const int32_t *query, int64_t n, int32_t rng_streams, uint64_t calls_before, uint32_t *rng_pos,
                       uint32_t *rng_seed, uint32_t *walk_pos, void *stream);

/* Sample n roots.  Outputs per root i, at fixed offsets i*stride (stride = bucket or M*m+1):
 *   set_ids [n*stride] int32   members in first-visit order (root first)
 *   set_keys[n*stride] uint64  packed LP row of each member
 *   nsize   [n]        int32   set size (<= stride)
 *   walks   [n*M*(m+1)] int32  (emit_walks only, else NULL)
 *   flags   [4]        int32   [0] |= 1 when RAND_R mode met a dead end (degree-0 non-root: the call
 *                              count is then data dependent and the stream cannot be reproduced in
 *                              parallel); [1] += roots whose set overflowed `bucket`; [3] |= 16 when a root
 *                              lies outside [0, num_nodes): it is never looked up (the reference reads out of
 *                              bounds there), its set is empty and the host mirror raises IndexError.
 *                              Caller zeroes.
 * rng_pos / rng_seed: from subgacc_rng_positions (RAND_R) or NULL (PHILOX). */
int subgacc_walk_sets(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                      const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                      int32_t *set_ids, uint64_t *set_keys, int32_t *nsize, int32_t *walks, int32_t *flags,
                      void *stream);

/* Fused form for the SpG pipeline: sample n roots and leave every set as a FINISHED SpG row at offset i*stride:
 *   row_ids [n*stride] int32  members sorted by node id (random_walks.py:79-80)
 *   row_slot[n*stride] int32  slot of the member's LP key in `uniq_table` (translate after subgacc_uniq_number)
 * The keys are registered in the table with tag (root_base+i)*stride + first-visit rank, which numbers the
 * distinct rows exactly like the reference's sequential pass (subg_acc.c:957-978); root_base = global index of
 * query[0] when a job is split into chunks.  Needs M*m+1 <= 818 (SUBGACC_ERR_LDS otherwise: use
 * subgacc_walk_sets + subgacc_compact_sets + subgacc_spg_build).  flags as for subgacc_walk_sets, [2] |= 1
 * when the table is (nearly) full. */
int subgacc_walk_spg(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                     const int32_t *query, int64_t n, int64_t root_base, const uint32_t *rng_pos,
                     const uint32_t *rng_seed, void *uniq_table, int64_t uniq_capacity, int32_t *row_ids,
                     int32_t *row_slot, int32_t *nsize, int32_t *flags, void *stream);
/* The same finished rows from the sets of subgacc_walk_sets (for the configurations where that kernel is the faster
 * walk -- short walks over a cache-resident graph): row i of the staging area, row_ids / row_keys [i*stride, +nsize[i])
 * in first-visit order, becomes (ids sorted by node id, slots in `uniq_table`) IN PLACE (row_ids) and in row_slot,
 * the LP keys registered with tag (root_base+i)*stride + first-visit rank -- one pass, instead of
 * subgacc_compact_sets + subgacc_uniq_number + subgacc_spg_build and a packed copy.  stride <= 1024. */
int subgacc_finish_rows(int32_t *row_ids, const uint64_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride,
                        int64_t root_base, void *uniq_table, int64_t uniq_capacity, int32_t *row_slot, int32_t *flags,
                        void *stream);
/* strided -> packed copy of the rows of subgacc_walk_spg: row i goes to [row_off[i], +nsize[i]).  With uniq_table
 * (already numbered by subgacc_uniq_number) out_data receives SFptr+1 directly; without it the raw table slots. */
int subgacc_compact_rows(const int32_t *row_ids, const int32_t *row_slot, const int32_t *nsize, const int64_t *row_off,
                         int64_t n, int32_t stride, int32_t *out_indices, int32_t *out_data, const void *uniq_table,
                         int64_t uniq_capacity, void *stream);

/* Exclusive scan int32 -> int64, out[n] = total.  (Prefix of nsize, subg_acc.c:848-851.) */
size_t subgacc_scan_workspace_bytes(int64_t n);
int subgacc_exclusive_scan_i32(const int32_t *in, int64_t n, int64_t *out, void *workspace, size_t workspace_bytes,
                               void *stream);

/* n <= 4,096 words of device memory (sizes, status words) to pinned, device-visible host memory by a one-wave kernel -- the read-back
 * of a lazily resolved step without a copy engine in the stream (the reference returns its sizes by value, subg_acc.c:1017-1024). */
int subgacc_publish_words(const int64_t *src, int64_t n, int64_t *host_dst, void *stream);

/* Left-compact the strided per-root sets (subg_acc.c:870-871): row i goes to [row_off[i], +nsize[i]).
 * out_keys may be NULL when uniq_table is given.  With uniq_table (see below; `uniq_capacity` slots) the pass
 * also inserts every member's key with position tag_base + row_off[i] + r (subg_acc.c:957-978) and writes the
 * table slot of every member to out_slot[] -- this replaces a separate subgacc_uniq_insert over out_keys. */
int subgacc_compact_sets(const int32_t *set_ids, const uint64_t *set_keys, const int32_t *nsize,
                         const int64_t *row_off, int64_t n, int32_t stride, int32_t *out_ids, uint64_t *out_keys,
                         void *uniq_table, int64_t uniq_capacity, int64_t tag_base, int32_t *out_slot, int32_t *flags,
                         void *stream);

/* ---------------------------------------------------------------------------------------------
 * Global first-occurrence dedup of LP rows (subg_acc.c:957-978): key -> index in order of first
 * appearance over the concatenated sets.  Open-addressing table in HBM, `capacity` a power of two.
 * Limits (tests/test_gpu_uniq_edges.py pins each of them):
 *   - the key 2^64 - 1 marks an empty slot and is NOT a key (subgacc_key_shift refuses the one (M, m) whose rows could pack to it);
 *   - a probe chain ends after 128 slots (or `capacity`, if smaller): the 129th key of one home slot, or the (capacity+1)-th
 *     distinct key, sets flags[2] |= 1 and is dropped -- grow the table and insert again; what was numbered meanwhile is void;
 *   - the scan numbering (more than `small_limit` distinct keys) recognises a first occurrence by mintag == its position in
 *     `slot`, so `slot` must be the concatenated out_slot of the inserts with positions EQUAL to the tags (tag_base + e); the
 *     direct ranking reads the table alone.  With n = 0 (slot may be NULL) and more than small_limit distinct keys, nothing is
 *     numbered: out_count is right, ids and out_ukeys are left as they were.
 * ------------------------------------------------------------------------------------------- */
size_t subgacc_uniq_table_bytes(int64_t capacity);
int subgacc_uniq_reset(void *table, int64_t capacity, void *stream);
/* insert keys[0..n) whose global element positions are tag_base+0..n-1 (the position the element has in the
 * concatenated `slot` array later handed to subgacc_uniq_number); out_slot[e] (optional) = table slot of
 * keys[e]; flags[2] |= 1 when the table is (nearly) full */
int subgacc_uniq_insert(void *table, int64_t capacity, const uint64_t *keys, int64_t n, int64_t tag_base,
                        int32_t *out_slot, int32_t *flags, void *stream);
/* number the distinct keys by first occurrence (ascending minimum position):
 *   out_ukeys[] uint64 the distinct keys in index order (at most max_unique are written)
 *   out_count   int64  number of distinct keys (device scalar)
 * Tables with at most `small_limit` (<=0: 8192) distinct keys are ranked directly; larger ones are numbered by
 * a scan over the n elements (`slot` = the out_slot of the inserts, positions == tags). */
size_t subgacc_uniq_number_workspace_bytes(int64_t capacity, int64_t n);
int subgacc_uniq_number(void *table, int64_t capacity, const int32_t *slot, int64_t n, uint64_t *out_ukeys,
                        int64_t max_unique, int64_t *out_count, int64_t small_limit, void *workspace,
                        size_t workspace_bytes, void *stream);
/* slot_inout[e] <- index of the element's key (+add): remap[1] of the reference with add = 0, the SpG payload
 * SFptr+1 with add = 1.  n_dev (optional, device scalar): process min(n, *n_dev) elements -- lets a caller that
 * has not read the element count back yet launch over its buffer capacity. */
int subgacc_uniq_translate(void *table, int64_t capacity, int32_t *slot_inout, int64_t n, const int64_t *n_dev,
                           int32_t add, void *stream);

/* Unpack keys to LP rows [n, m+1]: col 0 = M on LEAD rows else 0 (subg_acc.c:751,982-1000).
 * out_i16 / out_i32 / out_f32 may each be NULL; out_f32 is float(count)/float(M) (main.py:174) and,
 * with zero_row != 0, gets an all-zero row prepended (random_walks.py:81) => [n+1, m+1].
 * n_dev (optional, device scalar): only the first min(n, *n_dev) keys are valid, later rows are zero-filled. */
int subgacc_unpack_lp(const uint64_t *keys, int64_t n, const int64_t *n_dev, int32_t num_walks, int32_t num_steps,
                      int16_t *out_i16, int32_t *out_i32, float *out_f32, int32_t zero_row, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SpG build (sampler/random_walks.py:79-80: scipy COO->CSR): sort each row's members by node id.
 *   out_indices[X] int32 sorted ids, out_data[X] int32 = sf+1.  With uniq_table != NULL, sf[] holds table slots
 *   (out_slot of the inserts) and is translated on the fly, after subgacc_uniq_number.
 *   max_len >= max nsize; a longer row is
 *   left unwritten and flags[3] |= 1 (flags: the int32[4] word array of subgacc_walk_sets).
 * ------------------------------------------------------------------------------------------- */
int subgacc_spg_build(const int64_t *row_off, int64_t n, const int32_t *ids, const int32_t *sf,
                      const void *uniq_table, int64_t uniq_capacity, int32_t max_len, int32_t *out_indices,
                      int32_t *out_data, int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SpJoin (train.py:13-45 gather, :48-72 hgather, :75-111 bgather/pgather).
 * A join is a list of S segments (own[j], partner[j]) of SpG row numbers: segment j emits one row
 * per member w of row own[j] in ascending id order with the pair
 *     ( value_own(w), value_partner(w) or 0 ).
 * gather(edge[2,B]):  own = [u..,v..], partner = [v..,u..];  hgather: [u,w,v,w] / [w,u,w,v].
 * ABI 4: with a mirrored list (pair_block > 0, see subgacc_join_desc) `partner` may be NULL in every fill entry point: the
 * partner of segment j is then the own row of j's mirror (own[j + pair_block] in an even block, own[j - pair_block] in an odd
 * one) -- gather() passes its [2,B] endpoint tensor as `own` as it stands and builds no second list.
 * ------------------------------------------------------------------------------------------- */
/* out_seg[S+1] int64 = exclusive scan of the segment sizes (`indptr` of train.py:20-22).
 * n_rows = rows of the store.  A row number outside [0, n_rows) in own / partner (partner may be NULL: not checked
 * then) -- an IndexError of `x[edge[0]]` in the reference, train.py:15 -- is never dereferenced by any join entry
 * point: the row reads as empty and flags[3] |= 16 (flags: int32[4], caller zeroes; may be NULL). */
size_t subgacc_sjoin_workspace_bytes(int64_t S);
int subgacc_sjoin_sizes(const int64_t *spg_indptr, int64_t n_rows, const int64_t *own, const int64_t *partner, int64_t S,
                        int64_t *out_seg, int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);
int subgacc_sjoin_sizes_rows(const int32_t *row_len, int64_t n_rows, const int64_t *own, const int64_t *partner, int64_t S,
                             int64_t *out_seg, int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);   /* strided rows */
/* the size pass of a star list (SUBGACC_JOIN_OPT_STAR below) over packed rows: own = the P sources, partner = the P*K targets,
 * S = 2*P*K segments; out_seg [2*P*K+1] is what subgacc_sjoin_sizes writes for the expanded list.  P*K < 2^31. */
int subgacc_sjoin_star_sizes(const int64_t *spg_indptr, int64_t n_rows, const int64_t *own, const int64_t *partner, int64_t P,
                             int64_t K, int64_t *out_seg, int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);

/* ONE entry point fills the R = out_seg[S] rows of every form of the join: the descriptor states what the store looks
 * like, what a member's payload is, which segments to join and which outputs are wanted; subgacc_sjoin_fill_v2 dispatches.
 * (Since ABI 7 it is the only fill entry point.)
 *
 *   store      exactly one of three row layouts.  PACKED rows: row_off [n_rows+1] (the SpG of random_walks.py:79).  STRIDED rows:
 *              row_len [n_rows] + row_stride (the form subgacc_walk_spg leaves a transient batch in -- row r = [r*row_stride,
 *              +row_len[r]) -- joined where they lie, no packed copy).  HEADED rows (ABI 7; row_off = row_len = NULL, row_stride > 1):
 *              a RESIDENT store on whole 128-byte lines (subgacc_rows_to_headed writes it; row_stride a multiple of 32) -- slot 0 of
 *              row r's ids, ids[r*row_stride], holds the row's LENGTH, its members follow at ids[r*row_stride + 1 + t], member t's
 *              payload is payload[r*row_stride + t]: a row needs no row pointer (its place is r*row_stride, its length arrives
 *              with its first members), begins on a line and ends inside its own last one -- what a packed store reads beyond
 *              the algorithmic bytes (rows that begin and end inside lines, a line per row pointer) is gone, for row_stride /
 *              (mean length) of its size.  ids: member ids, ascending inside a row; max_len >= the longest row touched (packed
 *              rows; a longer row sets flags[3] |= 1 and its segment is skipped; strided rows: row_stride is the bound, headed
 *              rows: row_stride - 1).  Mirrored lists of rows that do not fit LDS (~13k members) and lists that are not mirrored
 *              take a one-segment-per-wave kernel (packed rows only); rows beyond that (~20k int / ~13k float members) are
 *              searched in place.
 *   payload    SUBGACC_JOIN_SFPTR  int32: SFptr+1 (packed rows) or a slot of `uniq_table` (strided rows: slots become SFptr+1 through
 *                                  the numbered table's id plane on their way in; uniq_table = NULL: `table` is indexed by slot+1
 *                                  itself, subgacc_unpack_lp(zero_row = 1)); feature rows are gathered from table f32 [table_rows, k]
 *                                  (Z_SF with the zero row; an SFptr outside it is never read: flags[3] |= 2)
 *              SUBGACC_JOIN_F64    double: the PPR encoder's score (train.py:39-43); xz is [R,2,1] = (float(own), float((partner or
 *                                  0.0) + 1.0 - 1.0)), the SciPy expression of train.py:33 in double.  Strided / headed rows: max_len is
 *                                  not a bound here but the number of members a row is asked for before its length is known
 *                                  (0 = min(row slot, 128))
 *              SUBGACC_JOIN_KEY32  int32 LP key (key = sum_j count_j << ((num_steps - j) * SHIFT), bit num_steps*SHIFT set on a root's
 *                                  own row, subg_acc.c:900-955): a feature row is the key's unpacked counts / num_walks -- what
 *                                  subgacc_unpack_lp writes into the feature table, computed on the fly (main.py:174's IEEE division);
 *                                  partner absent = the zero row.  Needs num_steps*SHIFT+1 <= 31.  Packed rows: a store re-keyed once
 *                                  (SpG.keyed); strided rows: what subgacc_walk_spg(uniq_table = NULL) writes
 *              SUBGACC_JOIN_KEY64  uint64 LP key: the strided rows of subgacc_walk_keyrows64 (4 hops, 32..63 bits); strided / headed rows
 *   segments   own / partner [S], seg [S+1] from subgacc_sjoin_sizes(_rows); pair_block = 0: independent segments (SFPTR / F64, packed
 *              rows); pair_block = P > 0: blocks of P segments, block 2t+1 mirrors block 2t (own / partner swapped) -- gather passes
 *              P = B, hgather P = B, nb batches at once P = B -- the two rows of a pair are read once and both blocks produced from
 *              there (flags[3] |= 4 if the list is not mirrored like that); `partner` may then be NULL.  Strided rows, keys, the count
 *              and the pair form: mirrored lists only
 *   form       SUBGACC_JOIN_ROWS   out_xz f32 [R,2,k] and / or out_idx i32 [R,2] (the raw index pairs, SFPTR only), out_segid i64 [R]
 *                                  (segment id of every row: `ptr=False`, train.py:25-30, and always for hgather's triplets,
 *                                  train.py:57-59; optional; every row layout and payload, the strided rows of an on-demand step --
 *                                  table slots, KEY32, KEY64 -- included: a row's id leaves with the span that carries the row)
 *              SUBGACC_JOIN_COUNTS out_counts f32 [S, table_rows]: how often LP row p (SFptr+1, 0 = partner absent) occurs in either
 *                                  feature slot of segment j, so that segment_sum_j(MLP(xz).sum(-2)) == out_counts[j] @ MLP(Z_SF)
 *                                  (model.py:78-83); 8*max_len + 8*table_rows + 16 bytes of LDS <= 160 KiB (SUBGACC_ERR_LDS)
 *              SUBGACC_JOIN_PAIRS  for aggregations that are not linear in the rows (the attention gate, model.py:59-62): segment j as
 *                                  its DISTINCT index pairs with multiplicities, in a reproducible order, at rows [seg[j], seg[j] +
 *                                  out_cnt[j]) of out_pairs i32 [R,2], out_mult i32 [R]; out_cnt i32 [S]; max_len <= 1024
 *   options    SUBGACC_JOIN_OPT_SIZES (row form): the WHOLE join of a batch in this one call -- the size pass runs first, as ONE
 *              launch, and the fill behind it.  seg = NULL; out_seg [S+1] is written (what subgacc_sjoin_sizes writes) and read by
 *              the fill; the outputs must hold the worst case (S * max_len rows, R is not known to the host beforehand); the size
 *              pass ORs its status into flags[3] (16: a row number outside the store; 64: size_state was not clean -- the segment pointers
 *              mean nothing, the fill of this call, and of every later one that finds the bit set, writes no row: zero the state
 *              and flags and call again); host_tail (optional; int64[2] of pinned, device-visible host memory) receives [R, the status of THIS
 *              size pass] when it ends (R = -1 with bit 64), so that a serving loop needs neither a memset in front of the join
 *              nor a copy behind it.  size_state: subgacc_sjoin_workspace_bytes(S) bytes of device memory the caller zeroes ONCE, when allocating
 *              it: every call leaves it zeroed again (a single-pass scan keeps its ticket and one word per tile there); one
 *              state serves one join at a time (calls on one stream; one state per stream otherwise).
 *              With NO output (out_xz = out_idx = NULL) the call is the size pass alone: out_seg and host_tail are written and
 *              nothing else -- the "count" half of a two-call pattern (then: allocate R rows, call again with seg = that out_seg
 *              and without the option) for callers that do not hold a worst-case buffer.
 *              SUBGACC_JOIN_OPT_STAR: a STAR list -- one source row against K target rows, the MRR evaluation of the reference
 *              (train.py:246-280 joins neg_edge = stack([source.repeat_interleave(K), target_neg.view(-1)]), utils.py:93-95), without
 *              the expanded [2, P*K] list: own = the P source rows, partner = the P*K target rows (target j belongs to source j / K),
 *              pair_block = K, S = 2*P*K.  The segments are the reference's: the left block [src(0) .. src(P*K-1)], then the right block
 *              [tgt(0) .. tgt(P*K-1)]; seg, out_xz, out_segid and flags mean exactly what they mean for gather over the expanded edge
 *              tensor (bit for bit the same rows).  The segment pointers come from subgacc_sjoin_star_sizes (packed rows) or, with
 *              OPT_SIZES as well, from the one-launch size pass (packed or headed rows).  Scope: the row form; packed and headed rows;
 *              payloads SFPTR, KEY32 and F64; out_xz (+ out_segid).  Refused with SUBGACC_ERR_BADARG before anything is launched:
 *              strided rows, KEY64, the count and pair forms, out_idx, pair_block <= 0, S not 2*P*K, partner = NULL.  A row number
 *              outside the store reads as an empty row and sets flags[3] |= 16, as for any other list.  A source row is staged in LDS
 *              once per workgroup of targets; a source too long for that (packed rows: ~13k members with a table, ~8k float members)
 *              is joined by the one-segment-per-wave kernel on the same list instead, with the same result.  flags[1] |= 1 when the
 *              star kernel ran, |= 2 when a source took that fallback.
 *   struct_bytes = sizeof(subgacc_join_desc); fields a form does not read must be zero / NULL.
 * Every entry point that takes this descriptor (subgacc_sjoin_fill_v2 and the fused stages below) refuses with SUBGACC_ERR_BADARG,
 * before anything is launched and with a message that starts with its name less the subgacc_ prefix ("sjoin_fill_v2: ..."): a NULL
 * descriptor; a descriptor of another size (struct_bytes); not exactly one row layout (both row_off and row_len, or neither with
 * row_stride <= 0); row_stride outside [1, 2^31) for strided rows or [2, 2^31) for headed rows; a negative S, n_rows or max_len.  The
 * fused stages, which join a mirrored list and write only outputs of their own, also refuse pair_block <= 0, S not a multiple of
 * 2*pair_block, own = NULL with S > 0, and any out_* or seg field of the descriptor set. */
enum { SUBGACC_JOIN_SFPTR = 0, SUBGACC_JOIN_F64 = 1, SUBGACC_JOIN_KEY32 = 2, SUBGACC_JOIN_KEY64 = 3 };
enum { SUBGACC_JOIN_ROWS = 0, SUBGACC_JOIN_COUNTS = 1, SUBGACC_JOIN_PAIRS = 2 };
enum { SUBGACC_JOIN_OPT_SIZES = 1, SUBGACC_JOIN_OPT_STAR = 2 };
typedef struct subgacc_join_desc {
    int32_t struct_bytes, form, payload_kind, max_len;
    const int64_t *row_off;
    const int32_t *row_len;
    int64_t row_stride, n_rows;
    const int32_t *ids;
    const void *payload;
    const void *uniq_table;
    int64_t uniq_capacity;
    const int64_t *own, *partner;
    int64_t S;
    const int64_t *seg;
    int64_t pair_block;
    const float *table;
    int64_t table_rows;
    int32_t k, num_walks, num_steps, options;
    float *out_xz;
    int32_t *out_idx;
    int64_t *out_segid;
    float *out_counts;
    int32_t *out_pairs, *out_mult, *out_cnt;
    int32_t *flags;
    int64_t *out_seg;           /* options & SUBGACC_JOIN_OPT_SIZES */
    void *size_state;
    int64_t size_state_bytes;
    int64_t *host_tail;
} subgacc_join_desc;
int subgacc_sjoin_fill_v2(const subgacc_join_desc *d, void *stream);
/* The same rows written as fp16 or bf16, for callers that train in mixed precision: a second header, include/subgacc_half.h */

/* The first model stage of the PPR / SPD / DEG encoders (utils.py:35-36 and main.py:170-196: a float payload, xz [R,2,1]) fused with
 * the join -- model.py:78-83, x = pe_embedding(xz).sum(dim=-2); xl, xr = MeanAggregation(x, ptr) -- for pe_embedding =
 * Sequential(Linear(1, H), ReLU, Linear(H, H')).  Mean aggregation is linear, so for segment j with n_j >= 1 rows (a_t, b_t)
 *     mean_t pe(a_t) + pe(b_t) = W2 M_j + 2 b2,   M_j[c] = (1/n_j) sum_t relu(fmaf(w1[c], a_t, b1[c])) + relu(fmaf(w1[c], b_t, b1[c]))
 * and the join writes only M (f32 [S, H]), not xz and the [R,2,H] activations.  (a_t, b_t) are bit for bit the rows the row form
 * writes: a = float(own), b = float((partner or 0.0) + 1.0 - 1.0) in double (train.py:33).  For the backward, out_p / out_q (both or
 * neither) receive  P_j[c] = (1/n_j) sum_t sum_{s in {a_t, b_t}} s [fmaf(w1[c], s, b1[c]) > 0]  and  Q_j[c] = (1/n_j) sum_t sum_s
 * [fmaf(w1[c], s, b1[c]) > 0]:  dL/dw1 = sum_j G_j * P_j, dL/db1 = sum_j G_j * Q_j with G = dL/dM (ReLU's gradient at 0 is 0).
 * Summation order, the same on every path (packed or headed rows, staged or streamed, every run): per channel c, the own row's members
 * in ascending id order, for each the a-term and then the b-term added to an fp32 sum starting at 0; then one IEEE division by n_j.
 * An empty segment (n_j = 0, or a row outside the store) gives zero rows in all three outputs.
 *   d        the descriptor of a mirrored row-form join of an F64 store: packed (row_off, max_len) or headed (row_stride) rows, own /
 *            partner (partner may be NULL), pair_block = P > 0, S = 2*P*nb, flags (int32[4], caller zeroes).  No size pass, no seg: a
 *            segment's size is its own row's length -- one launch.
 *   w1, b1   f32 [H]: Linear(1, H)'s weight and bias (a zero b1 for a Linear without bias); 1 <= H <= 1024.
 * Flags as the row form: flags[3] |= 16 a row number outside the store, |= 1 a packed row longer than max_len, |= 4 a list that is
 * not mirrored (the segments of such a pair are not written); flags[1] |= 2 when a pair had a row too long to stage (1,024 members)
 * and streamed.  Refused with SUBGACC_ERR_BADARG before anything is launched, besides the descriptor refusals of every fused stage
 * (subgacc_join_desc): a payload other than F64, strided rows, form != ROWS or any option bit, w1 / b1 / out_mean NULL, H outside
 * [1, 1024], exactly one of out_p / out_q, headed rows the row form refuses. */
int subgacc_sjoin_relu_mean(const subgacc_join_desc *d, const float *w1, const float *b1, int32_t H, float *out_mean,
                            float *out_p, float *out_q, void *stream);

/* The same first stage with attentional aggregation (--aggr attn: model.py:59-62,78-81, torch_geometric 2.2's
 * AttentionalAggregation(gate_nn, nn) with one-Linear gate_nn (wg, bg) and nn).  Every step after r_t is affine: for segment j with
 * rows (a_t, b_t), r_t[c] = relu(fmaf(w1[c], a_t, b1[c])) + relu(fmaf(w1[c], b_t, b1[c])) and x_t = W2 r_t + 2 b2, the gate is
 * u . r_t + (a constant softmax drops) with u = W2^T wg, and out_j = nn(W2 A_j + 2 b2) [n_j > 0] with A_j the softmax-weighted mean of
 * r_t.  The join writes only (f32 [S, H])
 *     A_j[c] = (sum_t e_t r_t[c]) / den_j,   e_t = expf(l_t - m_j),  l_t = u . r_t,  m_j = max_t l_t,  den_j = sum_t e_t
 * and, when the backward is wanted, out_max / out_den (both or neither; f32 [S]) receive m_j and den_j.  (den_j >= 1, so PyG's
 * den + 1e-16 is den in fp32.)  (a_t, b_t) are the rows the row form writes, as for subgacc_sjoin_relu_mean.
 * Summation order, the same on every path (packed or headed rows, staged or streamed, every run): l_t = an fp32 fmaf chain over c
 * ascending from 0, l = fmaf(u[c], r_t[c], l), r_t[c] the a-term plus the b-term; den_j and every A_j[c] (acc = fmaf(e_t, r_t[c],
 * acc)) over the own row's members in ascending id order from 0, then one IEEE division; m_j a max (order-free); expf, never __expf.
 * An empty segment (n_j = 0, or a row outside the store) gives a zero row and m_j = den_j = 0.
 *   d        as subgacc_sjoin_relu_mean's (a mirrored row-form join of an F64 store, packed or headed rows, no seg, no out_*).
 *   w1, b1   f32 [H]: Linear(1, H)'s weight and bias (a zero b1 for a Linear without bias); u f32 [H]; 1 <= H <= 1024.
 * Flags as subgacc_sjoin_relu_mean's: flags[3] |= 16 a row outside the store, |= 1 a packed row longer than max_len, |= 4 a list that is
 * not mirrored; flags[1] |= 2 a pair with a row longer than 1,024 members streamed (one pass for m_j, one for den_j and A_j).
 * Refused with SUBGACC_ERR_BADARG before anything is launched, besides the descriptor refusals of every fused stage (subgacc_join_desc):
 * a payload other than F64, strided rows, form != ROWS or any option bit, w1 / b1 / u / out_a NULL, H outside [1, 1024], exactly one
 * of out_max / out_den, headed rows the row form refuses. */
int subgacc_sjoin_relu_attn(const subgacc_join_desc *d, const float *w1, const float *b1, const float *u, int32_t H, float *out_a,
                            float *out_max, float *out_den, void *stream);

/* The backward of subgacc_sjoin_relu_attn over the same descriptor: g = dL/dA, a = A, max / den = m, den as the forward wrote them.
 * The pair is joined again and r_t, e_t recomputed bit for bit; alpha_t = e_t / den_j, beta_t = alpha_t (G_j . r_t - G_j . A_j) (both
 * dot products fmaf chains over c ascending), dr_t[c] = fmaf(alpha_t, G_j[c], beta_t u[c]).  Written per segment (f32 [S, H], no
 * atomics: dL/du = sum_j Du_j, dL/dw1 = sum_j Dw_j, dL/db1 = sum_j Db_j):
 *     Du_j[c] = sum_t beta_t r_t[c],  Dw_j[c] = sum_t dr_t[c] (a_t [ya > 0] + b_t [yb > 0]),  Db_j[c] = sum_t dr_t[c] ([ya > 0] + [yb > 0])
 * with ya = fmaf(w1[c], a_t, b1[c]), yb likewise (ReLU's gradient at 0 is 0), each an fmaf chain over the own row's members in
 * ascending id order from 0; an empty segment gives zero rows.  Flags and refusals as the forward's; g, a, max, den and the three
 * outputs are required. */
int subgacc_sjoin_relu_attn_backward(const subgacc_join_desc *d, const float *w1, const float *b1, const float *u, int32_t H,
                                     const float *g, const float *a, const float *max, const float *den, float *out_dw, float *out_db,
                                     float *out_du, void *stream);

/* The LP encoder's first stage with attentional aggregation (--aggr attn: model.py:59-62,78-81, one-Linear gate_nn (wg, bg) and nn)
 * fused with the count form of the join.  Member t of segment j is the index pair (p_t, q_t) -- SFptr+1 of the member in its own row,
 * in the partner row or 0 (SUBGACC_JOIN_COUNTS) -- and its row is E[p_t] + E[q_t] with E = pe_embedding(Z_SF) [T, H], so with
 * g = E wg (f32 [T]; the gate bias is a constant the softmax drops) the gate logit is l_t = g[p_t] + g[q_t] and, the weights summing to
 * 1, out_j = nn(W[j] @ E) [n_j > 0] with the softmax-weighted count row
 *     W[j, r] = (sum_t e_t ([p_t = r] + [q_t = r])) / den_j,   e_t = expf(l_t - m_j),  m_j = max_t l_t,  den_j = sum_t e_t
 * written densely (f32 [S, T], zeros where r does not occur in segment j); out_max / out_den (both or neither; f32 [S]) receive m_j
 * and den_j for the backward.  Neither xz, nor the [R,2,H] activations, nor the pair rows exist.
 * Summation order, the same on every path (either row of a pair staged, every run): l_t = one fp32 add; m_j a max (order-free); expf,
 * never __expf; den_j an fp32 chain over the own row's members in ascending id order from 0; for each r, sum_t e_t c_t(r) an fp32 chain
 * over the same members in the same order, adding e_t if p_t = r and then again if q_t = r; then one IEEE division by den_j.  No float
 * is added atomically.  An empty segment (n_j = 0, or a row outside the store) gives a zero row and m_j = den_j = 0.
 *   d        a count-form descriptor: form = SUBGACC_JOIN_COUNTS, payload SUBGACC_JOIN_SFPTR, packed rows (row_off, max_len), own /
 *            partner (partner may be NULL), pair_block = P > 0, S = 2*P*nb, table_rows = T, flags (int32[4], caller zeroes); no out_*
 *            field, no seg, no option bit.
 *   g        f32 [T].
 * Flags as the count form: flags[3] |= 1 a packed row longer than max_len, |= 2 an SFptr outside the table (read as row 0, never out of
 * bounds), |= 4 a list that is not mirrored (the segments of such a pair are not written), |= 16 a row number outside the store.
 * Refused with SUBGACC_ERR_BADARG before anything is launched, besides the descriptor refusals of every fused stage (subgacc_join_desc):
 * form != COUNTS or any option bit, a payload other than SFPTR, strided or headed rows, table_rows outside [1, 2^31), g / out_w NULL,
 * exactly one of out_max / out_den.  LDS: 4 (7 max_len + 2 T + 2 D + 8) bytes, D = min(2 max_len, T) (the backward: 6 D) <= 160 KiB,
 * else SUBGACC_ERR_LDS (the pair form, attn_stage, has no such bound); with out_max / out_den given a backward follows, so the
 * backward's LDS must fit too, else SUBGACC_ERR_LDS before anything is launched. */
int subgacc_sjoin_counts_attn(const subgacc_join_desc *d, const float *g, float *out_w, float *out_max, float *out_den, void *stream);

/* The backward of subgacc_sjoin_counts_attn over the same descriptor: dw = dL/dW, w = W, max / den = m, den as the forward wrote them.
 * The pair is joined again and e_t recomputed bit for bit; dw is read only at the segment's own LP rows.  With
 *     kappa_j = sum_r W[j, r] dW[j, r]   an fmaf chain over the rows r that occur in segment j, r ascending, from 0,
 *     beta_t = alpha_t ((dW[j, p_t] + dW[j, q_t]) - kappa_j),   alpha_t = e_t / den_j  (one add, one subtraction, one product),
 * out_dg (f32 [S, T]) receives per segment  Dg_j[r] = sum_t beta_t ([p_t = r] + [q_t = r])  in the forward's order (members in ascending
 * id order from 0, beta_t if p_t = r, then again if q_t = r), zeros elsewhere; dL/dg = sum_j Dg_j (no atomics).  An empty segment gives
 * a zero row.  Flags and refusals as the forward's; g, dw, w, max, den and out_dg are required. */
int subgacc_sjoin_counts_attn_backward(const subgacc_join_desc *d, const float *g, const float *dw, const float *w, const float *max,
                                       const float *den, float *out_dg, void *stream);

/* The LP encoder's first stage with LSTM aggregation (--aggr lstm: model.py:63-65,78-83, PyG's LSTMAggregation: to_dense_batch, a
 * one-layer batch_first nn.LSTM, the output at the last position), folded over the index form of the join (ABI 7, backward compatible
 * additions).  Segment j is the rows [indptr[j], indptr[j+1]) of pairs (p_t, q_t) -- SFptr+1 of the member in its own row, in the
 * partner row or 0 -- and row t's input is E[p_t] + E[q_t] with E = pe_embedding(Z_SF) [T, H].  The input projection folds into the
 * table G = E W_ih^T (f32 [T, 4H'], gate order i, f, g, o as nn.LSTM's) and b = b_ih + b_hh (f32 [4H'], NULL = zero).  Every segment
 * runs exactly L steps from h = c = 0, as the reference's zero padding makes it: step t < n_j takes G[p_t] + G[q_t], steps
 * n_j <= t < L take zero input (an empty segment runs L padded steps); a segment longer than L runs its first L rows only (n_j =
 * min(length, L)) and its later rows are ignored.  out_h (f32 [S, H']) receives h_{L-1}.  Per step and element:
 *     a = ((G[p_t] + G[q_t]) + b) as the accumulator's initial value (0 + b on a padded step), then + W_hh[row] . h_{t-1} as an fmaf
 *         chain over k ascending (v_mfma_f32_16x16x4_f32, bit for bit such a chain);
 *     i = 1 / (1 + expf(-a_i)), f, o likewise, g = tanhf(a_g) (accurate expf / tanhf, never the fast intrinsics);
 *     c_t = (f c_{t-1}) + (i g),  h_t = o tanhf(c_t)   (each product rounded, no fma).
 * A segment's bits depend only on its own rows and on L: not on the segments that share its tile, the pair order or the store layout.
 * h_state / c_state (both or neither; f32 [S, L, H']) receive every h_t, c_t for the backward ([j][t][k]; 8 S L H' bytes).
 * A pair index outside [0, T) reads row 0 and sets flags[3] |= 2 (flags int32[4], caller zeroes); nothing is read out of bounds.
 * Refused with SUBGACC_ERR_BADARG before anything is launched: pairs / indptr / G / w_hh / out_h / flags NULL, S < 0, L < 1 with S > 0,
 * H' not a multiple of 16 or outside [16, 128], T < 1, exactly one of h_state / c_state. */
int subgacc_lstm_aggr(const int32_t *pairs, const int64_t *indptr, int64_t S, int32_t L, int64_t T, int32_t H, const float *G,
                      const float *b, const float *w_hh, float *out_h, float *h_state, float *c_state, int32_t *flags, void *stream);

/* The backward of subgacc_lstm_aggr (BPTT, t = L-1 .. 0): dh = dL/dh_{L-1} (f32 [S, H']), h_state / c_state as the forward wrote them.
 * The gates are recomputed bit for bit (the forward's order); dh_{t-1} = W_hh^T dgates_t is an fmaf chain over the 4H' gate rows
 * ascending.  No float is added atomically:
 *   out_dw (f32 [ceil(S/16), 4H', H']) / out_db (f32 [ceil(S/16), 4H']): one partial per tile of 16 segments (dL/dW_hh, dL/db = their
 *            sums over tiles); inside a tile dW_hh[n][k] is an fmaf chain over t descending and, per step, the tile's segments in the
 *            order 4i + s (MFMA i = 0..3, s = 0..3); db per lane quad over t descending of (((d_0 + d_1) + d_2) + d_3), the 4 quads added
 *            in order.  Padded steps contribute here only.
 *   ws_rows (f32 [R, 4H'], R = indptr[S]): dgates of every real row, in row order; rows past L of a segment longer than L take no
 *            step and receive zeros, so dG ignores them as the forward does (every row of ws_rows is written).
 *   out_dg (f32 [T, 4H']): dL/dG[r] = the sum of ws_rows over the 2R index entries (row, side) with index r, in the order `order`
 *            lists them: order (int32 [2R]) holds the row of every entry of a stable sort of the 2R indices; piece_off (int64
 *            [n_pieces + 1]) cuts it into pieces inside one index's run; run_piece (int64 [T + 1]): the pieces of index r are
 *            [run_piece[r], run_piece[r+1]).  Each piece is summed from 0 in order into ws_pieces (f32 [n_pieces, 4H']), then each
 *            index's pieces are summed from 0 in order.
 * Flags and refusals as the forward's; h_state, c_state, dh, order, piece_off, run_piece, ws_rows, out_dg, out_dw and out_db are
 * required, ws_pieces when n_pieces > 0; n_pieces outside [0, 2^31) is refused. */
int subgacc_lstm_aggr_backward(const int32_t *pairs, const int64_t *indptr, int64_t S, int32_t L, int64_t T, int32_t H, const float *G,
                               const float *b, const float *w_hh, const float *h_state, const float *c_state, const float *dh,
                               const int32_t *order, const int64_t *piece_off, int64_t n_pieces, const int64_t *run_piece,
                               float *ws_rows, float *ws_pieces, float *out_dg, float *out_dw, float *out_db, int32_t *flags,
                               void *stream);

/* The float encoders' (PPR / SPD / DEG) first stage with LSTM aggregation in the same recurrent kernel (ABI 7, backward compatible
 * additions).  A row of the float join is a pair of scalars (a_t, b_t) -- own score, partner's score or 0 -- and pe_embedding =
 * Linear(1, H), ReLU, Linear(H, H1), so with V = W_ih W2 the input projection is  F(a_t) + F(b_t) + c_real,  F(s) = V relu(w1 s + b1):
 * a piecewise-linear function of ONE scalar.  Over the H knots -b1/w1 sorted ascending, F(s) = P[k] s + Q[k] in interval k of K = 2H + 1:
 * with r = the number of knots <= s (torch.bucketize, right=True), k = 2r in the open interval behind r knots and k = 2r - 1 ON a knot,
 * where that knot's channels count as off (F is continuous there; the gradients then take relu'(0) = 0 as torch does).  The caller
 * builds idx, P and Q by this one rule.  vals (f32 [R, 2]) holds (a_t, b_t), idx (int32 [R, 2]) their intervals,
 * tab (f32 [K, 4H', 2]) the pairs (P[k][n], Q[k][n]) interleaved, c_real = b_ih + b_hh + 2 W_ih b2 and c_pad = b_ih + b_hh (f32 [4H']
 * each, NULL = zero); vals, idx and tab on 8-byte boundaries.  Segments, L, padding, out_h, h_state / c_state, the MFMA chain over W_hh
 * and the cell update are those of subgacc_lstm_aggr; only the accumulator's initial value differs, per step and element:
 *     a = (fmaf(P[ka], a_t, Q[ka]) + fmaf(P[kb], b_t, Q[kb])) + c_real   on a real step,   a = 0 + c_pad   on a padded step.
 * A segment's bits depend only on its own rows, L and the tables: not on its tile-mates, the pair order or packed against headed rows.
 * An interval outside [0, K) reads row 0 and sets flags[3] |= 2; nothing is read out of bounds.
 * Refused with SUBGACC_ERR_BADARG before anything is launched: vals / idx / indptr / tab / w_hh / out_h / flags NULL, vals / idx / tab
 * off an 8-byte boundary, S < 0, L < 1 with S > 0, H' not a multiple of 16 or outside [16, 128], K outside [1, 2^22] (the table is addressed with 32-bit
 * offsets), exactly one of h_state / c_state. */
int subgacc_lstm_aggr_hinge(const float *vals, const int32_t *idx, const int64_t *indptr, int64_t S, int32_t L, int64_t K, int32_t H,
                            const float *tab, const float *c_real, const float *c_pad, const float *w_hh, float *out_h, float *h_state,
                            float *c_state, int32_t *flags, void *stream);

/* The backward of subgacc_lstm_aggr_hinge: BPTT as subgacc_lstm_aggr_backward runs it (gates recomputed bit for bit, out_dw and
 * ws_rows as there).  What differs, still without a float added atomically:
 *   out_dc_real / out_dc_pad (f32 [ceil(S/16), 4H'] each): the bias partials of a tile kept apart -- the dgates of real steps in
 *            out_dc_real, those of padded steps in out_dc_pad (they reach different parameters), each summed as out_db is, a step
 *            that belongs to the other sum adding 0.
 *   out_dp / out_dq (f32 [K, 4H'] each): dL/dP[k] = sum of ws_rows[row] * vals[row][side] and dL/dQ[k] = sum of ws_rows[row] over the 2R
 *            entries (row, side) with idx = k, in the order `order` lists them: order (int32 [2R]) holds the ENTRY 2 row + side of a
 *            stable sort of the 2R intervals (R < 2^30), piece_off / run_piece cut it as in subgacc_lstm_aggr_backward (K in T's place).
 *            Each piece is summed from 0 in order -- dP as the chain fmaf(d, val, .), dQ as plain adds -- into ws_pieces (f32
 *            [2, n_pieces, 4H']: dP's pieces, then dQ's), then each interval's pieces are summed from 0 in order.
 * Flags and refusals as the forward's; h_state, c_state, dh, order, piece_off, run_piece, ws_rows, out_dp, out_dq, out_dw, out_dc_real
 * and out_dc_pad are required, ws_pieces when n_pieces > 0; n_pieces outside [0, 2^31) is refused. */
int subgacc_lstm_aggr_hinge_backward(const float *vals, const int32_t *idx, const int64_t *indptr, int64_t S, int32_t L, int64_t K,
                                     int32_t H, const float *tab, const float *c_real, const float *c_pad, const float *w_hh,
                                     const float *h_state, const float *c_state, const float *dh, const int32_t *order,
                                     const int64_t *piece_off, int64_t n_pieces, const int64_t *run_piece, float *ws_rows,
                                     float *ws_pieces, float *out_dp, float *out_dq, float *out_dw, float *out_dc_real,
                                     float *out_dc_pad, int32_t *flags, void *stream);


/* Packed rows -> headed rows (ABI 7): the resident store of a serving loop laid out on whole lines -- the rows random_walks.py:79-81
 * builds as a SciPy CSR and train.py:17-18 / :39-43 slice one by one (x[edge[0]]), in the layout the pair kernels read with one
 * dependent trip less.  row_off [n+1], ids, payload
 * (payload_bytes = 4: SFptr+1 / 32-bit keys, 8: PPR scores / 64-bit keys) as SpG holds them; out_ids [n*row_stride] int32 and
 * out_payload [n*row_stride] of the same element size, row_stride >= (longest row) + 1 (a longer row is cut and flags[3] |= 1), a
 * multiple of 32 for rows on whole 128-byte lines.  Slots behind a row's members are left as they are. */
int subgacc_rows_to_headed(const int64_t *row_off, int64_t n_rows, const int32_t *ids, const void *payload, int32_t payload_bytes,
                           int64_t row_stride, int32_t *out_ids, void *out_payload, int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Top-K approximate-PPR node sets -- replaces sampler/pprgo.py:9-38 (_calc_ppr_node, the
 * Andersen-Chung-Lang push with a LIFO work list), :53-63 (calc_ppr_topk_parallel), :85-111 (topk_ppr_matrix
 * normalisation) and utils.py:35-36 (encoding 'PPR').  The graph is an unweighted CSR without repeated entries
 * in a row (deg = row length, as np.sum(adj > 0, 1) / adj.sum(1) of pprgo.py:69,92 give for such a graph).
 * The push order and every float32 rounding follow the reference (numba typing: alpha, epsilon, p, r float32;
 * (1 - alpha) * res / deg in float64, rounded on the store), so rows are reproducible bit for bit; equal scores
 * at the top-k cut keep the node that entered p later.
 *
 * One wavefront works on one root at a time in a private `slab` of 24 << table_log2 bytes (hash table of p, r
 * and the work list).  num_waves slabs = num_waves resident wavefronts; reset the slabs once, the kernel hands
 * them back clean (table_log2 in [10, 26]).  A root that touches T nodes in all (itself, the pushed nodes and their neighbours)
 * always fits when 2 * T + 257 <= 1 << table_log2 and never when T + 256 > 3 / 4 of the table; 1/(alpha*epsilon) bounds the
 * pushed nodes, not T (one push of a hub touches deg + 1 nodes; T <= num_nodes).  A root that does not fit
 * gets out_count = -1 and flags[2] |= 1: run those roots again with a larger table.
 *   out_count [n] int32, out_ids [n*topk] int32 ascending ids of row i at i*topk, out_vals [n*topk] float32
 *   pushes (optional, device uint64[2]) accumulates the number of pushes and of touched nodes.  topk <= 4096.
 * ------------------------------------------------------------------------------------------- */
size_t subgacc_ppr_slab_bytes(int32_t table_log2, int32_t num_waves);
int subgacc_ppr_slab_reset(void *slab, int32_t table_log2, int32_t num_waves, void *stream);
int subgacc_ppr_topk(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes,
                     const int32_t *roots, int64_t n, float alpha, float epsilon, int32_t topk, void *slab,
                     int32_t table_log2, int32_t num_waves, int32_t *out_count, int32_t *out_ids, float *out_vals,
                     int32_t *flags, uint64_t *pushes, void *stream);
/* Packed rows (row_off[n+1], ids, vals) -> float64 payload.  mode 0 'row': unchanged; 1 'sym':
 * sqrt(max(deg_root,1e-12)) * v * (1/sqrt(max(deg_col,1e-12))); 2 'col': deg_root * v * (1/max(deg_col,1e-12))
 * (pprgo.py:88-108, evaluated left to right in float64).  max_nnz >= row_off[n] sizes the launch.  max_bits
 * (optional, device uint64, zeroed by the caller) receives the bit pattern of the largest output value. */
int subgacc_ppr_normalize(const void *indptr, int32_t indptr64, const int32_t *roots, int64_t n,
                          const int64_t *row_off, int64_t max_nnz, const int32_t *ids, const float *vals, int32_t mode,
                          double *out, uint64_t *max_bits, void *stream);
/* utils.py:35-36: data = (data + 0.1) / (max + 0.1) over the first *nnz_dev entries; max from max_bits. */
int subgacc_ppr_encode(double *data, int64_t max_nnz, const int64_t *nnz_dev, const uint64_t *max_bits, void *stream);

/* ---------------------------------------------------------------------------------------------
 * DEG and SPD structural encoders over a PPR node-set store (utils.py:22-34, `encoding(x, adj, 'DEG' | 'SPD')`):
 * per row the union of the PPR row x_i (x_off / x_ids / x_val, ids ascending) and the adjacency row N(i), with
 *   mode 1 DEG  value(i,j) = log(|x_j u N(j)| + 1)  (log_table[d] = log(d+1), made by the caller with the libm the
 *               reference uses); out_agg(i,j) = x_ij + 1/deg(i)  (`x += normalize(adj, 'l1')`, the `agg` return)
 *   mode 2 SPD  value(i,j) = 1[j in N(i)] + 0.5[j in x_i and N(i) n N(j) != {}] + 0.3[j in x_i], diagonal = 2.3
 *               (x1 + x0.multiply(x1**2 * 0.5) + x0 * 0.3; setdiag(2.3)); the adjacency is taken as symmetric.
 * Rows = nodes (n = number of nodes), adjacency rows ascending without repeats.  Two calls: subgacc_encode_sizes
 * gives row_len[n] (for DEG these are also the d of the value rule); scan them into out_off[n+1]; then
 * subgacc_encode_fill writes the merged rows (ids ascending) -- kmax >= longest x row (<= 8192).
 * flags[3] |= 8: a row length outside log_table.
 * ------------------------------------------------------------------------------------------- */
int subgacc_encode_sizes(const int64_t *x_off, const int32_t *x_ids, int64_t n, const void *indptr, int32_t indptr64,
                         const int32_t *indices, int32_t mode, int32_t *row_len, int32_t *flags, void *stream);
int subgacc_encode_fill(const int64_t *x_off, const int32_t *x_ids, const double *x_val, int64_t n, int32_t kmax,
                        const void *indptr, int32_t indptr64, const int32_t *indices, int32_t mode,
                        const int32_t *deg_row_len, const double *log_table, int64_t log_len, const int64_t *out_off,
                        int32_t *out_ids, double *out_val, double *out_agg, int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * walk_join of the legacy SUREL surface (subg_acc/subg_acc.c:509-647): for every query pair (a, b) of roots and
 * every position t of their raw walks, the running index of the visited node in a's key list and in b's key list
 * (find_idx, :78-92; 0 = absent).
 *   walks   int32 [n, stride]           raw walks, row i belongs to root i (walk_sampler's first output)
 *   set_*   the n key lists as SpG-form rows: set_off int64[n+1], set_ids int32 ascending per row, set_idx int32 =
 *           1 + position of the member in the concatenation of the lists as given (:573-584) -- what
 *           subgacc_spg_build makes of (row_off, ids, sf = 0..X-1)
 *   qrow    int32 [Q,2] row numbers of the query keys (find_key_item, :617; -1 = not a root: that pair yields -1s)
 *   out     int32 [2, Q*2*stride], 8-byte aligned: out[s][2*x*stride + 2*t + {0,1}] = index of walks[row_s(x)][t] in
 *           the list of {key1, key2} of pair x  (:621-629)
 * max_len >= longest key list (sizes the LDS staging; rows past 5120 members are searched in place).
 * ------------------------------------------------------------------------------------------- */
int subgacc_walk_join(const int32_t *walks, int64_t n, int32_t stride, const int64_t *set_off, const int32_t *set_ids,
                      const int32_t *set_idx, int32_t max_len, const int32_t *qrow, int64_t Q, int32_t *out,
                      void *stream);

/* ---------------------------------------------------------------------------------------------
 * Key rows: a batch that is sampled, joined and dropped needs neither the table of distinct LP rows nor their numbering.
 * subgacc_walk_spg with uniq_table = NULL writes the member's 32-bit LP key itself as the row's payload (needs
 * num_steps*SHIFT+1 <= 31, 2 to 4 hops, set_sampler order, no bucket, M <= 256: SUBGACC_ERR_BADARG otherwise); such rows are
 * joined with payload SUBGACC_JOIN_KEY32 (subgacc_join_desc): same (xz, seg) as the table path, sizes by subgacc_sjoin_sizes_rows.
 * A PACKED store whose payload was re-keyed once (SpG.keyed) is joined the same way: for the reference's flow -- subg_matrix over all
 * nodes once, main.py:172-178, then one join per training batch, train.py:120-127 -- that takes the gather from the Z_SF table out of
 * every output row; xz is bit-identical to the SFPTR join with table = float32(enc) / num_walks, main.py:174.
 *
 * ABI 5 -- key rows for the 4-hop configurations.  The paper's sampler figure is citation2 with m = 4, M = 200 (Fig. 6a): its LP
 * key -- the reference's 64-bit `bithash`, subg_acc.c:900-955 -- takes 4 x 8 + 1 = 33 bits.  subgacc_walk_spg(uniq_table = NULL)
 * serves 2 to 4 hops while num_steps*SHIFT+1 <= 31 (4 hops: M <= 127, e.g. the reference's own citation2 setting M = 100,
 * README.md:82-96); beyond that, subgacc_walk_keyrows64 writes the same rows with the whole 64-bit key as payload:
 *   row_ids [n*stride] int32 (sorted by node id), row_keys [n*stride] uint64, nsize [n]; stride = M*m+1.
 * Shapes: 4 hops, 32 <= num_steps*SHIFT+1 <= 63, a 1,024-slot table (M*4+1 <= 818), set_sampler order, no bucket.  worklist /
 * n_work: optional (both or neither), as for subgacc_walk_spg_list / _sparse (rows that are not listed are left alone: zero nsize
 * first); rng_pos / rng_seed as for subgacc_walk_spg.  Joined with payload SUBGACC_JOIN_KEY64: bit for bit the xz of the table path.
 * ------------------------------------------------------------------------------------------- */
int subgacc_walk_keyrows64(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                           const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                           const int32_t *worklist, const int64_t *n_work, int32_t *row_ids, uint64_t *row_keys,
                           int32_t *nsize, int32_t *flags, void *stream);
/* ---------------------------------------------------------------------------------------------
 * Prologue of one on-demand step (sample both endpoints of B query pairs -> rows -> SpJoin; train.py:120-127 calls the
 * join once per batch of main.py:32's 1,024 pairs) in ONE launch: subgacc_uniq_reset of the table of distinct LP rows,
 * `n_zero` status words zeroed, and the n = 2B endpoints `edge` (int64, [u.. | v..]) narrowed to the int32 roots the
 * sampler takes (an id outside int32 becomes -1: out of range for the walk kernel, which flags it).
 * ------------------------------------------------------------------------------------------- */
int subgacc_step_prologue(void *uniq_table, int64_t capacity, int64_t *zero_words, int64_t n_zero, const int64_t *edge,
                          int32_t *roots, int64_t n, void *stream);   /* uniq_table may be NULL (key rows: no table) */

/* The same prologue for a step that samples every DISTINCT endpoint once.  Philox keys a walk by (seed, root id, walk, hop), so a
 * root's set does not depend on where or how often the root stands in the batch (the reference samples every node once, offline,
 * main.py:172-178; its sequential rand_r stream has no such property, so this form is Philox only).  Three launches (the first one
 * returns at once but for one step in 2^32 - 1, see `workspace`):
 *   roots       int32 [n]: roots[j] = endpoint j where j is the FIRST occurrence of its node in the batch, SUBGACC_NO_ROOT
 *               elsewhere -- rows of the batch's sets stay where the plain step has them, the rows of repeated endpoints
 *               stay empty (subgacc_walk_spg_sparse passes over them), and the distinct LP rows keep their numbering
 *   own, partner int64 [n]: gather()'s mirrored segment lists over those rows -- own[j] = row of endpoint j's first occurrence,
 *               partner[j] = that of the other end of its pair (j +- n/2); for subgacc_sjoin_sizes_rows / subgacc_sjoin_fill_v2 (strided rows)
 *   worklist    int32 [n]: the first occurrences, worklist[0 .. *n_distinct), in order of arrival (not reproducible, and it does
 *               not matter: entry k names its row) -- what subgacc_walk_spg_sparse runs over
 *   row_len     int32 [n]: the rows' lengths (the sampler's nsize): set to 0 for the rows of repeated endpoints, which the
 *               sampler will not visit
 *   n_distinct  int64 [1] (device): the number of distinct endpoints = the length of the work list
 *   workspace   subgacc_step_dedup_workspace_bytes(n) bytes, ZEROED once by the caller before its first use and left alone
 *               afterwards: it keeps the stamp of the last step (slots are stamped, not cleared from step to step), so a captured
 *               (replayed) step works like a launched one.  Its first int64 IS that stamp: the low 32 bits count the steps made on
 *               this workspace, 1, 2, .. 0xFFFFFFFF (0 = never used, and skipped afterwards).  The step after stamp 0xFFFFFFFF
 *               clears the table on the device, in a launch that is a no-op in every other step, and takes stamp 1: an era of
 *               2^32 - 1 steps ends and the next one starts from the zeroed state, with no host read and no action of the caller's
 *               (two months of 1.1 ms steps on one workspace).  The rest of the workspace has no documented layout.
 * The work list's ORDER is unspecified (compare it as a set); everything else the call writes is a function of `edge` alone.
 * ------------------------------------------------------------------------------------------- */
#define SUBGACC_NO_ROOT (-2147483647 - 1)
size_t subgacc_step_dedup_workspace_bytes(int64_t n);
int subgacc_step_prologue_dedup(void *uniq_table, int64_t capacity, int64_t *zero_words, int64_t n_zero, const int64_t *edge,
                                int32_t *roots, int64_t *own, int64_t *partner, int32_t *worklist, int32_t *row_len, int64_t n,
                                void *workspace, size_t workspace_bytes, int64_t *n_distinct, void *stream);
/* The dedup prologue for a step whose roots play ROLES: the n = r*B roots `edge` come in r blocks of B and the segment list has s
 * blocks of B, each reading one root block.  r = 3, s = 4: the triplets (u, v, w) of the higher-order model, edge = [u.. | v.. | w..],
 * segment blocks u, w, v, w -- hgather's [U|w ; W|u ; V|w ; W|v] (train.py:48-72), whose negatives keep (u, v) of their positive and
 * replace w (dataloader.py:265-268, 275: two of the three roots of every negative are repeats).  r = 2, s = 2: gather's pairs, blocks
 * u, v (train.py:13-23).  Written: roots, worklist, row_len and n_distinct as by subgacc_step_prologue_dedup -- first occurrence is
 * over the WHOLE root list, so a node that is u of one triplet and w of another is walked once -- and
 *   own         int64 [s*B]: own[b*B + t] = the row of the first occurrence of the root that segment t of block b reads
 * No partner list: the segment list is mirrored (pair_block = B: block 2t+1 mirrors block 2t), subgacc_sjoin_sizes_rows and
 * subgacc_sjoin_fill_v2 take partner = NULL.  workspace: subgacc_step_dedup_workspace_bytes(n) bytes, zeroed once, as above.
 * Refused before anything is launched, with a message that starts with "step_prologue_dedup_roles: ": a NULL argument
 * (SUBGACC_ERR_BADARG; uniq_table may be NULL: key rows), (r, s) other than (2, 2) and (3, 4), B <= 0, n != r*B or n >= 2^30, a
 * workspace that is too small (SUBGACC_ERR_WORKSPACE).
 * (The plain triplet step needs no entry point of its own: subgacc_step_prologue with n = 3B, and own = [0..B | 2B..3B | B..2B |
 * 2B..3B) is a constant of B.) */
int subgacc_step_prologue_dedup_roles(void *uniq_table, int64_t capacity, int64_t *zero_words, int64_t n_zero, const int64_t *edge,
                                      int32_t *roots, int64_t *own, int32_t *worklist, int32_t *row_len, int64_t n, int64_t B,
                                      int32_t r, int32_t s, void *workspace, size_t workspace_bytes, int64_t *n_distinct,
                                      void *stream);
/* subgacc_walk_spg over some of the rows only: the rows worklist[0 .. *n_work) (both on the device; the launch covers n rows,
 * blocks past the list's length leave at once), or -- worklist = n_work = NULL -- every row i whose query[i] is not
 * SUBGACC_NO_ROOT (such a row gets nsize[i] = 0 and nothing else is touched; rows that are not on the work list are not touched
 * at all).  Philox mode, set_sampler order, shapes the fused-row kernel serves (2..4 hops, M <= 256, M*m+1 <= 818, no bucket):
 * SUBGACC_ERR_BADARG otherwise.  Row i belongs to query[i]; tags of the table of distinct rows start at 0. */
int subgacc_walk_spg_sparse(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                            const int32_t *query, int64_t n, const int32_t *worklist, const int64_t *n_work, void *uniq_table,
                            int64_t uniq_capacity, int32_t *row_ids, int32_t *row_slot, int32_t *nsize, int32_t *flags,
                            void *stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 4 -- batched registration of key rows: the table of distinct LP rows (subg_acc.c:957-978) for a store that is KEPT
 * (subg_matrix, sampler/random_walks.py:74-82; main.py:172-178 samples all N nodes once), built from the rows of the fast
 * key-rows form of subgacc_walk_spg (uniq_table = NULL) instead of inside every root's walk:
 *   1. subgacc_keyrows_register: one pass over the rows' 32-bit LP keys (row i = row_keys[i*stride, +nsize[i])); every
 *      distinct key of a row goes to `uniq_table` with the COARSE tag (root_base+i)*stride + stride-1, and the rows whose
 *      insert lowered a key's tag -- the candidates for a key's first appearance, always including the true one -- are
 *      listed in cand[0 .. *n_cand) (int32 row numbers in arrival order; cand holds n entries, *n_cand is a device counter
 *      the caller zeroes);
 *   2. subgacc_walk_tags: the candidates alone (worklist = cand, *n_work = *n_cand; the launch covers min(n, work_cap)
 *      rows, work_cap = 0: n; a longer list raises flags[3] |= 32) are walked again by the table form of the fused-row
 *      kernel, which lowers their keys' tags to the exact (root_base+i)*stride + first-visit number and writes nothing
 *      else -- after it every distinct key carries the tag subgacc_walk_spg(uniq_table) would have given it, and
 *      subgacc_uniq_number numbers the table like the reference's sequential pass;
 *   3. subgacc_keyrows_compact: strided key rows -> packed rows at row_off[i] (the CSR copy of the store).  With `ukeys`
 *      (out_ukeys / out_count / max_unique of subgacc_uniq_number: one chunk of roots -- steps 1, 2, the numbering, then
 *      this) the payload is SFptr+1, looked up on the way.  With ukeys = NULL (a job of several chunks, numbered at the
 *      end) the pass registers the chunk's keys itself (as step 1, candidates listed; step 2 follows) and keeps the KEY as
 *      payload; subgacc_keyrows_translate turns the packed payloads of all chunks into SFptr+1 once the table is numbered
 *      (n_dev, optional: only the first min(n, *n_dev) entries).
 * Shapes: what the key-rows form of subgacc_walk_spg serves (num_steps*SHIFT+1 <= 31, 2 to 4 hops, M <= 256, no bucket).
 * rng_pos / rng_seed as for subgacc_walk_spg (RAND_R: positions of ALL n roots of the chunk; row i reads entry i).
 * cand: subgacc_keyrows_cand_capacity(n) entries (cand_cap says how many there are; every row is listed at most once).
 * Limits (tests/test_gpu_keyrows_edges.py pins each of them):
 *   - the 32-bit pattern 0xFFFFFFFF marks a free entry of the pass's dictionary and is NOT a key (the shapes above keep bit 31
 *     clear); any other pattern is a key, zero-extended to 64 bits in `uniq_table` and `ukeys` -- with bit 31 set it is a negative
 *     int32 as row_keys entry and as the payload of the ukeys = NULL form;
 *   - nsize[i] > stride is read as `stride`; row_off must be the prefix sum of those clamped lengths;
 *   - cand lists a SUPERSET of the rows that show a key first, each row once, in arrival order: which other rows it lists, and the
 *     order, differ from run to run; entries at and beyond *n_cand are not written.  The look-up form (ukeys != NULL) touches
 *     neither cand nor *n_cand nor the table;
 *   - the look-up form and subgacc_keyrows_translate read min(*n_ukeys, max_ukeys) entries of ukeys and ask `uniq_table` (numbered
 *     by subgacc_uniq_number, which numbers every key whatever max_unique says) for any other key; a key that is in no table
 *     gives the payload 0; subgacc_keyrows_translate leaves the entries at and beyond min(n, *n_dev) as they are;
 *   - more distinct keys than `uniq_table` takes (see the limits of subgacc_uniq_insert): flags[2] |= 1, every call still returns
 *     and writes its outputs only, and what was registered, numbered or copied meanwhile is void. */
int64_t subgacc_keyrows_cand_capacity(int64_t n);
int subgacc_keyrows_register(const int32_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride,
                             int64_t root_base, void *uniq_table, int64_t uniq_capacity, int32_t *cand, int64_t cand_cap,
                             int64_t *n_cand, int32_t *flags, void *stream);
int subgacc_walk_tags(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                      const int32_t *query, int64_t n, int64_t root_base, const uint32_t *rng_pos, const uint32_t *rng_seed,
                      const int32_t *worklist, const int64_t *n_work, int64_t work_cap, void *uniq_table,
                      int64_t uniq_capacity, int32_t *flags, void *stream);
int subgacc_keyrows_compact(const int32_t *row_ids, const int32_t *row_keys, const int32_t *nsize, const int64_t *row_off,
                            int64_t n, int32_t stride, int64_t root_base, void *uniq_table, int64_t uniq_capacity,
                            const uint64_t *ukeys, const int64_t *n_ukeys, int64_t max_ukeys, int32_t *out_indices,
                            int32_t *out_data, int32_t *cand, int64_t cand_cap, int64_t *n_cand, int32_t *flags, void *stream);
int subgacc_keyrows_translate(int32_t *data_inout, int64_t n, const int64_t *n_dev, void *uniq_table, int64_t uniq_capacity,
                              const uint64_t *ukeys, const int64_t *n_ukeys, int64_t max_ukeys, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The count form over the key rows of an on-demand step (ABI 7, backward compatible additions).  A step that samples, joins and drops
 * its batch (subgacc_walk_spg with uniq_table = NULL: rows of 32-bit LP keys) has neither the table of distinct LP rows nor their
 * numbering, which the count form of the join -- and with it the mean first stage, model.py:78-83 as (C @ MLP(Z_SF)) / sizes -- indexes
 * its columns by.  These two entry points give the step both, without xz [R,2,k] and without a resident store.
 *
 * subgacc_keyrows_columns: one column per DISTINCT LP key of the rows row_keys[i*stride, +nsize[i]), i < n (the strided key rows of a
 * step; a length beyond `stride` is read as `stride`), for table_rows = T >= 2 columns, column 0 being "partner absent":
 *   out_ukeys  int32 [T-1]    the distinct keys of all rows, ascending as unsigned integers (entries past the count: 0)
 *   out_count  int64 [1]      their number c, on the device
 *   out_feat   f32 [T, m+1]   row 0 zero (random_walks.py:81); row 1+i = out_ukeys[i] unpacked as subgacc_unpack_lp does it (float(count) /
 *                             float(M), main.py:174; column 0 = 1 on a root's own row): bit for bit the rows of xz; rows past c zero
 * A column is the RANK of its key among the batch's distinct keys -- not a hash slot, not a first-occurrence number (subg_acc.c:957-978
 * numbers by first appearance: a function of the order of the roots) --, so columns, counts and everything computed from them are the
 * same bits for every schedule, walk order and root dedup.  More than T-1 distinct keys: flags[2] |= 1 (the meaning this word has for a
 * full table of distinct rows), out_count = T-1, the T-1 smallest keys are kept (unless even the set of 2T..4T slots overflowed: then
 * some T-1 keys) and nothing is written out of bounds.  flags: int32[4], caller zeroes.
 * Two launches (a streaming pass that dedups per workgroup in LDS and inserts the survivors into a set in HBM; one workgroup that
 * sorts and unpacks), no host read, no allocation: capturable.  workspace: subgacc_keyrows_columns_workspace_bytes(T) bytes (0 for a
 * T the call refuses), ZEROED ONCE by its owner before the first call -- every call leaves it zeroed for the next (one workspace serves
 * one stream at a time).
 * Refused before anything is launched, with a message that starts with "keyrows_columns: ": T < 2, n < 0, stride <= 0, num_walks or
 * num_steps < 1, a key of more than 31 bits (num_steps*SHIFT+1 > 31), a NULL out_ukeys / out_count / out_feat / flags / workspace, NULL
 * row_keys / nsize with n > 0 (SUBGACC_ERR_BADARG); T > 16,384 (the keys are sorted in LDS: SUBGACC_ERR_LDS); a workspace that is too
 * small (SUBGACC_ERR_WORKSPACE). */
size_t subgacc_keyrows_columns_workspace_bytes(int64_t table_rows);
int subgacc_keyrows_columns(const int32_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride, int32_t num_walks,
                            int32_t num_steps, int64_t table_rows, int32_t *out_ukeys, int64_t *out_count, float *out_feat,
                            int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);

/* subgacc_sjoin_key_counts: SUBGACC_JOIN_COUNTS over those rows -- out_counts f32 [S, T] is exactly what the count form writes for an
 * SFptr store whose LP row 1+i is ukeys[i]: entry [j, 1+i] = how often key ukeys[i] occurs in either feature slot of segment j, entry
 * [j, 0] = the members of segment j without a partner, columns past *n_keys zero; so segment_sum_j(MLP(xz).sum(-2)) == out_counts[j] @
 * MLP(out_feat) (model.py:78-83; HONet, model_horder.py:56-57, with own = [u | w | v | w], S = 4B).  out_len (optional; int32 [S])
 * receives the length of every segment's own row, the mean's divisor.
 *   d        payload_kind = SUBGACC_JOIN_KEY32, strided rows (row_len, row_stride, ids, payload = the keys), own / partner (partner may
 *            be NULL), pair_block = P > 0, S a multiple of 2*P (any number of mirrored blocks: segment j = (p / P) * 2 * P + p % P of pair
 *            p), table_rows = T, num_walks, num_steps, flags (int32[4], caller zeroes); no out_* field, no seg, no option bit.
 *   ukeys    int32 [T-1] ascending (unsigned), n_keys int64 [1] on the device: out_ukeys / out_count of subgacc_keyrows_columns (at most
 *            min(*n_keys, T-1) keys are read).
 * The plan of the count form: the longer row of a pair staged, the shorter searched in it once, a hit counted for both blocks, n - hits
 * added to column 0; the sorted keys lie in LDS and every member's key is mapped to its column once, by a halving search; integer LDS
 * histograms, no float is added atomically.  Flags: flags[3] |= 2 a key that is not in the list (the feature slot that carries it is not counted; nothing
 * is read or written out of bounds), |= 1 a row longer than row_stride, |= 4 a list that is not mirrored (the segments of such a pair are
 * not written), |= 16 a row number outside the store (an empty row).  LDS: 8 row_stride + 12 T + 16 bytes <= 160 KiB, else
 * SUBGACC_ERR_LDS before anything is launched.  Refused with SUBGACC_ERR_BADARG before anything is launched, besides the descriptor
 * refusals of every fused stage (subgacc_join_desc): packed or headed rows, a payload other than KEY32, any option bit, T < 2, a NULL
 * ukeys / n_keys / out_counts. */
int subgacc_sjoin_key_counts(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, float *out_counts,
                             int32_t *out_len, void *stream);

/* subgacc_sjoin_key_counts_attn / _backward: the count form with attentional aggregation (subgacc_sjoin_counts_attn / _backward: the LP
 * encoder's first stage for --aggr attn, model.py:59-62,78-81) over those rows -- out_w f32 [S, T] is what subgacc_sjoin_counts_attn
 * writes for an SFptr store whose LP row 1+i is ukeys[i], bit for bit.  Member t of segment j is the index pair (p_t, q_t):
 *     p_t = 1 + the rank of its own key in ukeys;   q_t = the same for the member of the partner row with the same id, 0 without one
 * and everything else is subgacc_sjoin_counts_attn's arithmetic in its order: l_t = g[p_t] + g[q_t] (one fp32 add), m_j a max
 * (order-free), e_t = expf(l_t - m_j) (never __expf), den_j and each sum_t e_t c_t(r) fp32 chains over the own row's members in ascending
 * id order from 0 (e_t added if p_t = r, then again if q_t = r), one IEEE division; the backward: kappa_j an fmaf chain over the
 * segment's occurring columns in ascending column order, beta_t = alpha_t ((dW[j, p_t] + dW[j, q_t]) - kappa_j), Dg_j[r] a chain in the
 * forward's order, dL/dg = sum_j Dg_j.  No float is added atomically; either row of a pair may be the staged one, the bits are the
 * same.  An empty segment gives a zero row and m_j = den_j = 0.  out_max / out_den (both or neither; f32 [S]) keep m_j and den_j for
 * the backward; out_len (optional; int32 [S]) receives the length of every segment's own row.
 *   d        as subgacc_sjoin_key_counts: form SUBGACC_JOIN_COUNTS, payload_kind SUBGACC_JOIN_KEY32, strided rows, own / partner (partner
 *            may be NULL), pair_block = P > 0, S a multiple of 2*P (any number of mirrored blocks), table_rows = T >= 2, num_walks,
 *            num_steps, flags (int32[4], caller zeroes); no out_* field, no seg, no option bit.
 *   ukeys / n_keys   out_ukeys / out_count of subgacc_keyrows_columns (at most min(*n_keys, T-1) keys are read; *n_keys < 0 reads none).
 *   g        f32 [T].
 * One 256-lane workgroup per mirrored pair: the sorted keys lie in LDS, every member's key is mapped to its column once by a halving
 * search, then the layout of subgacc_sjoin_counts_attn's kernel.  Flags: flags[3] |= 2 a key that is not in the list (that slot is read
 * as column 0, as subgacc_sjoin_counts_attn reads an SFptr outside the table; nothing is read or written out of bounds), |= 1 a row
 * longer than row_stride, |= 4 a list that is not mirrored (the segments of such a pair are not written), |= 16 a row number outside
 * the store (an empty row).
 * LDS: 4 (7 row_stride + 3 T + 2 D + 7) bytes, D = min(2 row_stride, T) (the backward: 6 D) <= 160 KiB, else SUBGACC_ERR_LDS with a
 * message that names table_rows and the row form; with out_max / out_den given a backward follows, so the backward's LDS must fit too,
 * else SUBGACC_ERR_LDS from the forward.  (row_stride = 608, T = 2,048: 51,356 B forward, 70,812 B backward.)
 * Refused before anything is launched, each message led by the function's name: every refusal of subgacc_sjoin_key_counts; a NULL g /
 * out_w; exactly one of out_max / out_den; for the backward a NULL g / dw / w / max / den / out_dg (SUBGACC_ERR_BADARG); the LDS bound. */
int subgacc_sjoin_key_counts_attn(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g, float *out_w,
                                  float *out_max, float *out_den, int32_t *out_len, void *stream);
int subgacc_sjoin_key_counts_attn_backward(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g,
                                           const float *dw, const float *w, const float *max, const float *den, float *out_dg,
                                           void *stream);

/* subgacc_sjoin_key_index: the index form of the row form over those rows -- out_idx of SUBGACC_JOIN_ROWS, which subgacc_sjoin_fill_v2
 * writes for SFPTR payloads only, under the numbering of subgacc_keyrows_columns.  It replaces gather(ptr=...)'s rows (train.py:25-30,109)
 * as the input of the LP encoder's LSTM aggregation (model.py:63-65: subgacc_lstm_aggr runs over these pairs and G = MLP(out_feat) W_ih^T).
 *   out_idx  int32 [R, 2], 8-byte aligned (a pair leaves as one 8-byte store), R = seg[S]: row seg[j] + t is the index pair (p_t, q_t) of member t of segment j's own row, members in
 *            ascending id order (gather()'s row order):
 *                p_t = 1 + the rank of its own key in ukeys;   q_t = the same for the member of the partner row with the same id, 0 without one
 *            so that out_feat[out_idx[r]] is, bit for bit, row xz[r] of the row form over the same key rows.
 *   out_len  optional, int32 [S]: the length of every segment's own row.
 *   d        as subgacc_sjoin_key_counts, with form SUBGACC_JOIN_ROWS: payload_kind SUBGACC_JOIN_KEY32, strided rows (row_len, row_stride,
 *            ids, payload = the keys), own / partner (partner may be NULL), pair_block = P > 0, S a multiple of 2*P, table_rows = T >= 2,
 *            num_walks, num_steps, flags (int32[4], caller zeroes); no out_* field, no seg field, no option bit.
 *   ukeys / n_keys   out_ukeys / out_count of subgacc_keyrows_columns (at most min(*n_keys, T-1) keys are read; *n_keys < 0 reads none).
 *   seg      int64 [S+1], as subgacc_sjoin_sizes_rows writes it over the same rows and lists: segment j has one output row per member
 *            of its own row.
 * One 256-lane workgroup per mirrored pair: the sorted keys lie in LDS and every member's key is mapped to its column once by a halving
 * search; the longer row of the pair is staged (ids, columns, one word per member for its partner's column), the shorter is searched in
 * it once -- a hit writes the shorter row's pair and leaves its column in the staged member's word --, and after a barrier the staged
 * row's pairs leave as coalesced 8-byte stores.  Either row may be the staged one, the output is the same; no atomics on outputs.
 * Flags: flags[3] |= 2 a key that is not in the list (that slot is written as column 0; nothing is read or written out of bounds), |= 1
 * a row longer than row_stride, |= 4 a list that is not mirrored (the segments of such a pair are not written), |= 16 a row number
 * outside the store (an empty row).
 * LDS: 12 row_stride + 4 T bytes <= 160 KiB, else SUBGACC_ERR_LDS with a message that names table_rows and the row form, before
 * anything is launched.  (row_stride = 608, T = 2,048: 15,488 B.)
 * Refused with SUBGACC_ERR_BADARG before anything is launched, each message led by "sjoin_key_index: ": every refusal of
 * subgacc_sjoin_key_counts; a form other than SUBGACC_JOIN_ROWS; a NULL ukeys / n_keys; a NULL seg / out_idx with S > 0;
 * an out_idx that is not 8-byte aligned. */
int subgacc_sjoin_key_index(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const int64_t *seg,
                            int32_t *out_idx, int32_t *out_len, void *stream);

/* ABI 4: subgacc_walk_spg over ALL n rows but in the order of a work list (worklist[0 .. *n_work) names every row once:
 * subgacc_worklist_by_root) -- either RNG mode: row i keeps its place in the batch AND in the rand_r stream (rng_pos[i] /
 * rng_seed[i] from subgacc_rng_positions over the n roots in batch order; NULL for Philox), only the order in which the kernel
 * takes the rows changes.  Tags of the table of distinct rows start at 0.  Shapes: any that subgacc_walk_spg takes with a
 * table of distinct rows -- where the fused-row kernel declines (a truncating bucket, M > 256, ...) the general kernel walks
 * the rows in batch order, which gives the same rows; key rows (uniq_table = NULL) need the fused-row kernel's shapes. */
int subgacc_walk_spg_list(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                          const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                          const int32_t *worklist, const int64_t *n_work, void *uniq_table, int64_t uniq_capacity,
                          int32_t *row_ids, int32_t *row_slot, int32_t *nsize, int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * batch_sampler of the legacy SUREL surface (subg_acc/subg_acc.c:391-507): one insertion-ordered set of nodes grown by
 * walking the roots one after the other (num_walks walks of num_steps nodes each, first hop without replacement,
 * one rand_r stream); root i stops walking once the set holds (i+1)*thld/n nodes (:474).
 *   seed_eff   the state the reference starts from: its `seed` argument + getpid() (:421)
 *   out        int32 [out_cap] nodes in insertion order; *out_count (device) receives their number.
 *              A sufficient out_cap is min(num_nodes, n*(num_walks*num_steps+1)).  flags[1] |= 1 when it was too small,
 *              flags[0] |= 1 when a walk reached a node without out-edges (the stream position of the later walks is then
 *              data dependent and not reproduced), flags[3] |= 16 for a root outside [0, num_nodes) (skipped).
 *   workspace  subgacc_batch_sampler_workspace_bytes(out_cap) bytes (the set's hash table)
 * One workgroup: the loop over roots is sequential by definition; walks, dedup and ordering inside a root are parallel.
 * ------------------------------------------------------------------------------------------- */
size_t subgacc_batch_sampler_workspace_bytes(int64_t out_cap);
int subgacc_batch_sampler(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes,
                          const int32_t *query, int64_t n, int32_t num_walks, int32_t num_steps, int32_t thld,
                          uint32_t seed_eff, int32_t *out, int64_t out_cap, int64_t *out_count, void *workspace,
                          size_t workspace_bytes, int32_t *flags, void *stream);

/* ABI 4: the rows 0 .. n-1 of a batch as a work list in ascending order of their root's id (1,024 buckets of consecutive
 * ids, any order inside a bucket; rows whose root is SUBGACC_NO_ROOT -- the repeated endpoints subgacc_step_prologue_dedup
 * marks -- are left out; *n_work = the rows listed) -- what subgacc_walk_spg_sparse / _list then runs over: roots that are neighbours in id
 * space (the same community of a graph with id locality) or equal (repeated endpoints) are walked at the same time on the
 * same XCD and share its L2.  The rows stay where they are; only the order of the walk changes, so no result does (the order
 * INSIDE a bucket is the arrival order of atomics and differs from run to run).  Two small launches; workspace =
 * subgacc_worklist_workspace_bytes(n) bytes, ZEROED ONCE by its owner before the first call -- every call leaves it zeroed for
 * the next (one workspace serves one stream at a time). */
size_t subgacc_worklist_workspace_bytes(int64_t n);
int subgacc_worklist_by_root(const int32_t *roots, int64_t n, int64_t num_nodes, int32_t *worklist, int64_t *n_work,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Graph-locality order (ABI 7, backward compatible additions).  The reference walks its roots in whatever order its loop takes
 * them (subg_acc.c:742-745) and nothing observable depends on that order: Philox keys a walk by (seed, root id, walk, hop), the
 * list-order walk entry points keep every row's rand_r stream position, and every row is written at its own index.  So the order
 * is free to serve the L2: roots of the same community walked at the same time share their lines.  subgacc_worklist_by_root
 * gets that only where ids carry locality; these two entry points build an order that does not rely on the ids.
 *
 * subgacc_locality_round: ONE round of a deterministic label propagation over the CSR, labels_in -> labels_out (int32 [num_nodes]
 * each, distinct buffers; start from label[v] = v).  Node v updates in round `round` iff (mix32(v) & 1) == (round & 1), where
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32, mod 2^32);
 * every other node copies its label.  An updating node with deg > 0 reads the labels of min(deg, cap) neighbours -- all of them if
 * deg <= cap, else those at positions j*deg/cap (64-bit integer arithmetic), j < cap -- and its own label once more; the new label
 * is the most frequent of these, ties to the smallest.  deg == 0: the label stays.  1 <= cap <= 64, round >= 0, num_nodes < 2^31;
 * SUBGACC_ERR_BADARG otherwise (checked before anything is launched).  Sorting the nodes by (final label, id) gives the order
 * (surel_plus_amd.sampler.locality_order; 8 rounds, cap = 64 by default).
 *
 * subgacc_worklist_by_rank: subgacc_worklist_by_root keyed by rank[root] instead of the root's id (rank: int32 [num_nodes] on the
 * device, e.g. the position of the node in that order): 1,024 buckets of consecutive ranks, any order inside a bucket; rows whose
 * root is SUBGACC_NO_ROOT are left out, a root outside [0, num_nodes) goes to the last bucket.  Same workspace contract as
 * subgacc_worklist_by_root (zeroed once by its owner, left zeroed by every call).
 * ------------------------------------------------------------------------------------------- */
int subgacc_locality_round(const void *indptr, int32_t indptr64, const int32_t *indices, int64_t num_nodes,
                           const int32_t *labels_in, int32_t *labels_out, int32_t round, int32_t cap, void *stream);
int subgacc_worklist_by_rank(const int32_t *roots, int64_t n, const int32_t *rank, int64_t num_nodes, int32_t *worklist,
                             int64_t *n_work, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGACC_H */
