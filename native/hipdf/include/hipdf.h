/* hipdf C ABI — the kernel surface of the MI355X columnar engine as plain
 * extern "C" functions over raw device pointers (reference analogue: the
 * JNI contract the Spark plugin holds against cudf-java, SURVEY.md §2.8A;
 * pybind (hipdf_module.cpp) is ONE consumer of this ABI, this header and
 * libhipdf.so let a JVM/C/C++ host be another).
 *
 * This header is the only declaration of the surface and it is complete:
 * every extern "C" function and every descriptor struct the library exports
 * is declared here and nowhere else. Every kernel translation unit and the
 * pybind module include it, so the compiler checks each definition and each
 * call against the one declaration ("conflicting types" on any drift).
 *
 * Column model (Arrow-style):
 *   - fixed-width column: device array of `size` values (HipdfType)
 *   - validity: uint64 words, bit i = row i valid; NULL => all valid
 *   - string column: int32 offsets[size+1] + uint8 bytes
 * All functions enqueue onto the given HIP stream and return immediately.
 * Unless a comment says otherwise: `av`/`bv`/`ov`/`*valid` are validity
 * words, `sel` is an optional int32 row selection (NULL = all rows), `ao`/
 * `ab` (`bo`/`bb`) are a string column's offsets and bytes, `row_gid` is
 * int32 group ids, and `out_off`/`out_len` are the int64 byte offsets and
 * lengths of a two-pass string producer (mode 0 = measure, 1 = write).
 */
#ifndef HIPDF_H
#define HIPDF_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define HIPDF_STATIC_ASSERT(cond, msg) static_assert(cond, msg)
extern "C" {
#else
#define HIPDF_STATIC_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif

typedef enum {
  HIPDF_U8 = 0,
  HIPDF_I8 = 1,
  HIPDF_I16 = 2,
  HIPDF_I32 = 3,
  HIPDF_I64 = 4,
  HIPDF_F32 = 5,
  HIPDF_F64 = 6,
} HipdfType;

/* Arrow-C-data-interface-shaped column descriptor for host bookkeeping.
 * Device kernels take the raw pointers below. */
typedef struct {
  int dtype;            /* HipdfType */
  int64_t size;         /* rows */
  const void* data;     /* device values (or string bytes) */
  const void* validity; /* device uint64 words or NULL */
  const void* offsets;  /* device int32[size+1] for strings, else NULL */
} HipdfColumnDesc;

/* ---- descriptor structs: filled by the caller, uploaded as device arrays.
 * The sizes are what python's struct.pack produces for them. ------------- */

/* multi-column row-equality descriptor for group-by / join builds */
typedef struct {
  int type;            /* HipdfType, or 7 for int128 (lo, hi) pairs */
  int is_string;       /* 1 -> data=int32* offsets, aux=uint8* bytes */
  const void* data;
  const uint64_t* valid;
  const void* aux;
} HipdfKeyCol;
HIPDF_STATIC_ASSERT(sizeof(HipdfKeyCol) == 32, "packed as <iiqqq");

/* one fixed-width column of hipdf_gather_table */
typedef struct {
  int esize;            /* element size in bytes */
  int in_has_valid;
  const void* in;
  const uint64_t* in_valid;
  void* out;
  uint64_t* out_valid;  /* may be null */
} HipdfGatherCol;
HIPDF_STATIC_ASSERT(sizeof(HipdfGatherCol) == 40, "packed as <iiqqqq");

/* one key of the dense group-id fast path (hipdf_dense_gid). idx == NULL: an
 * integer key column, row i reads vals[i] of `type` under `valid`. idx set:
 * a code-table key, vals is an int32 table and row i reads vals[idx[i]];
 * idx[i] < 0 takes the NULL slot, `type` and `valid` are not looked at. */
typedef struct {
  int type;        /* HipdfType of the key column */
  int pad;
  const void* vals;
  const uint64_t* valid;
  int64_t kmin;
  int64_t range;   /* #distinct slots for values; NULL takes index `range` */
  int64_t stride;
  const int32_t* idx;  /* may be null; int32 rows of the table `vals` */
} HipdfDenseKey;
HIPDF_STATIC_ASSERT(sizeof(HipdfDenseKey) == 56, "packed as <iiqqqqqq");

/* one aggregate of the fused hipdf_gb_agg_multi */
typedef struct {
  int op;             /* 0 sum 1 min 2 max 3 count 4 count_all */
  int type;           /* HipdfType of the value column */
  int acc_is_double;  /* accumulator: double (1) or int64 (0) */
  int skip_cnt;       /* sum/min/max over a non-null column: the count
                       * atomic is pure overhead (group validity is
                       * implied by group existence) — skip it in the
                       * global-atomic path; the LDS path still counts
                       * (its flush is gated on lcnt) */
  const void* vals;
  const uint64_t* valid;
  void* acc;          /* [ngroups] double or int64 */
  int64_t* cnt;       /* [ngroups] */
} HipdfAggDesc;
HIPDF_STATIC_ASSERT(sizeof(HipdfAggDesc) == 48, "packed as <iiiiqqqq");

/* one input column of hipdf_str_concat_ws */
typedef struct {
  const int32_t* off;
  const uint8_t* bytes;
  const uint64_t* valid;
} HipdfStrColDesc;
HIPDF_STATIC_ASSERT(sizeof(HipdfStrColDesc) == 24, "packed as <qqq");

/* Host-side description of one sort key column for hipdf_sort_order; the
 * array of these stays in host memory. */
typedef enum {
  SORT_KEY_FIXED = 0,      /* one u64 key per row from a HipdfType column */
  SORT_KEY_STRING = 1,     /* nchunks 8-byte big-endian chunks, last first */
  SORT_KEY_DECIMAL128 = 2, /* interleaved (lo, hi) int64 pairs: lo then hi */
} HipdfSortKind;

typedef struct {
  int32_t kind;        /* HipdfSortKind */
  int32_t htype;       /* HipdfType of data (fixed keys only) */
  const void* data;    /* values; string bytes for SORT_KEY_STRING */
  const void* valid;   /* validity bitmask, or null */
  const void* offsets; /* int32 string offsets (SORT_KEY_STRING only) */
  int32_t desc;
  int32_t nulls_last;
  int32_t has_valid;   /* the column carries a validity mask */
  int32_t nchunks;     /* ceil(max string length / 8), at least 1 */
} HipdfSortKey;
HIPDF_STATIC_ASSERT(sizeof(HipdfSortKey) == 48, "two ints, three pointers, "
                                                "four ints");

/* ---- elementwise (kernels/elementwise.hip) ----------------------------- */
/* ops: 0 add 1 sub 2 mul 3 div ... (see _BIN_OPS in
 * spark_rapids_amd/ops/gpu_backend.py); scalar_rhs: b is the scalar sd/si */
void hipdf_binary_arith(int op, int t, const void* a, const void* b,
                        double sd, int64_t si, int scalar_rhs, const void* av,
                        const void* bv, void* out, void* ov, int64_t n,
                        hipStream_t stream);
/* out: uint8[n] */
void hipdf_binary_cmp(int op, int t, const void* a, const void* b, double sd,
                      int64_t si, int scalar_rhs, const void* av,
                      const void* bv, void* out, void* ov, int64_t n,
                      hipStream_t stream);
/* a, b, out: uint8 booleans; sb: the scalar when scalar_rhs */
void hipdf_binary_bool(int op, const void* a, const void* b, int sb,
                       int scalar_rhs, const void* av, const void* bv,
                       void* out, void* ov, int64_t n, hipStream_t stream);
void hipdf_unary(int op, int t, const void* a, const void* av, void* out,
                 void* ov, int64_t n, hipStream_t stream);
void hipdf_cast(int from_t, int to_t, const void* a, void* out, int64_t n,
                hipStream_t stream);
void hipdf_f64_to_i64_rint(const void* a, void* out, int64_t n,
                           hipStream_t stream);
/* int64 unscaled decimals: multiply by pow10 (up) or divide by it, rounding
 * half up */
void hipdf_decimal_rescale(const void* a, void* out, int64_t pow10, int up,
                           int64_t n, hipStream_t stream);
/* cond: uint8[n] with validity cv; rows where cond is true AND valid take
 * a, else b */
void hipdf_if_else(int t, const void* cond, const void* cv, const void* a,
                   const void* av, const void* b, const void* bv, void* out,
                   void* ov, int64_t n, hipStream_t stream);
/* validity words -> uint8[n] */
void hipdf_mask_expand(const void* mask, void* out, int invert, int64_t n,
                       hipStream_t stream);

/* ---- selection (kernels/selection.hip) --------------------------------- */
/* list offsets int32[nrows+1] -> per child element its row id and position
 * (both int32) */
void hipdf_expand_rows(const void* offsets, void* rowid, void* pos,
                       int64_t nrows, hipStream_t stream);
int64_t sel_num_blocks(int64_t n);
/* per-block popcounts of a uint8 boolean mask (mvalid may be NULL) */
void hipdf_mask_count(const void* mask, const void* mvalid,
                      void* block_counts /* int64[sel_num_blocks] */,
                      int64_t n, hipStream_t stream);
/* emit the selected row indices given exclusive per-block offsets */
void hipdf_mask_scatter(const void* mask, const void* mvalid,
                        const void* block_offsets, void* out_idx /* int32 */,
                        int64_t n, hipStream_t stream);
/* idx: int32[n_out] */
void hipdf_gather_fixed(int esize, const void* in, const void* idx, void* out,
                        int64_t n_out, hipStream_t stream);
/* in, out: int32 dictionary codes; a negative index yields the code -1 */
void hipdf_gather_codes(const void* in, const void* idx, void* out,
                        int64_t n_out, hipStream_t stream);
/* cols: device HipdfGatherCol[ncols]; a negative index yields a null */
void hipdf_gather_table(const void* cols, int ncols, const void* idx,
                        int64_t n_out, hipStream_t stream);
void hipdf_gather_validity(const void* in_valid, int in_has_valid,
                           const void* idx, void* out_valid, int64_t n_out,
                           hipStream_t stream);
/* lens: int64[n_out] */
void hipdf_gather_str_lens(const void* offsets, const void* idx, void* lens,
                           int64_t n_out, hipStream_t stream);
/* out_offsets: int64[n_out] byte offsets into out_bytes */
void hipdf_gather_str_bytes(const void* in_bytes, const void* in_offsets,
                            const void* idx, const void* out_offsets,
                            void* out_bytes, int64_t n_out,
                            int64_t total_bytes, hipStream_t stream);
void hipdf_narrow_i64_i32(const void* in, void* out, int64_t n,
                          hipStream_t stream);
/* copy n validity bits of src to bit offset dst_off of dst */
void hipdf_copy_valid_range(const void* src, int src_has_valid,
                            int64_t dst_off, void* dst, int64_t n,
                            hipStream_t stream);

/* ---- scan / reduce (kernels/scan.hip) ---------------------------------- */
int64_t scan_num_blocks(int64_t n);
/* int64 in/out; sums: int64[scan_num_blocks(n)] */
void hipdf_scan_block(const void* in, void* out, void* sums, int64_t n,
                      hipStream_t stream);
void hipdf_scan_add_offsets(void* out, const void* scanned_sums, int64_t n,
                            hipStream_t stream);
/* scratch elements hipdf_exclusive_scan_i64 needs for n inputs: per level
 * above the first, the block sums and their scan; the top level's single
 * block sum (the grand total) comes last. */
int64_t scan_scratch_elems(int64_t n);
/* All levels of the exclusive scan of in[0, n) -> out, enqueued on `stream`
 * without synchronising. scratch holds scan_scratch_elems(n) int64; its last
 * element receives the grand total. */
void hipdf_exclusive_scan_i64(const void* in, void* out, void* scratch,
                              int64_t n, hipStream_t stream);
/* the same, doing nothing when byte (skip_shift / 8) of the device u64 *skip
 * is zero (the radix sort's constant-digit passes); skip may be NULL */
void hipdf_exclusive_scan_i64_skip(const void* in, void* out, void* scratch,
                                   int64_t n, const void* skip,
                                   int skip_shift, hipStream_t stream);
/* op: 0 sum 1 min 2 max 3 count; acc: one double (float types) or int64,
 * acc_count: int64[1], both initialised by the caller */
void hipdf_reduce(int op, int t, const void* a, const void* av, void* acc,
                  void* acc_count, int64_t n, hipStream_t stream);

/* ---- hashing (kernels/hash.hip) ---------------------------------------- */
/* kind: 0 int32-like, 1 int64-like, 2 float, 3 double (spark murmur3);
 * seeds: int32[n] initialized with the seed, updated in place */
void hipdf_murmur3_col(int kind, int t, const void* a, const void* av,
                       const void* sel, void* seeds, int64_t n,
                       hipStream_t stream);
void hipdf_murmur3_str(const void* offsets, const void* bytes, const void* av,
                       const void* sel, void* seeds, int64_t n,
                       hipStream_t stream);
/* as murmur3, seeds: int64[n] */
void hipdf_xxhash64_col(int kind, int t, const void* a, const void* av,
                        const void* sel, void* seeds, int64_t n,
                        hipStream_t stream);
void hipdf_xxhash64_str(const void* offsets, const void* bytes,
                        const void* av, const void* sel, void* seeds,
                        int64_t n, hipStream_t stream);
/* h: int32 hashes -> part: int32 pmod(h, nparts) */
void hipdf_pmod_part(const void* h, int nparts, void* part, int64_t n,
                     hipStream_t stream);

/* ---- digests (kernels/digest.hip) --------------------------------------- */
/* md5 / sha1 / sha2 of each row's bytes as lowercase hex, thread per row.
 * Row i's W digits go to out_bytes + i * W (W = 32, 40, 56, 64, 96, 128 by
 * algo), so the result's offsets are i * W; a null row gets W '0' digits.
 * out_bytes: n * W bytes, 16-byte aligned. */
void hipdf_digest_hex(int algo, const void* offsets, const void* bytes,
                      const void* av, void* out_bytes, int64_t n,
                      hipStream_t stream);
    /* algo: 0 md5, 1 sha1, 2 sha224, 3 sha256, 4 sha384, 5 sha512 */
/* crc32 (zlib) of each row's bytes, unsigned, widened: out_i64 int64[n];
 * a null row writes 0 */
void hipdf_crc32_str(const void* offsets, const void* bytes, const void* av,
                     void* out_i64, int64_t n, hipStream_t stream);

/* ---- group-by (kernels/groupby.hip) ------------------------------------ */
/* CAS hash build over a power-of-two slot table (cap slots, slot_row
 * int32[cap] initialized to -1); claimed_slots int32[n]; ngroups int32[1]
 * zero-initialized */
void hipdf_gb_build(const void* hashes, const void* keys /* HipdfKeyCol[] */,
                    int nkeys, const void* sel, void* slot_row,
                    void* row_slot, void* claimed_slots, void* ngroups,
                    int64_t cap, int64_t n, hipStream_t stream);
/* slot_gid: int32[cap]; leaders: int32[max_groups], a row of each group */
void hipdf_gb_number(const void* claimed_slots, const void* slot_row,
                     void* slot_gid, const void* ngroups, void* leaders,
                     int64_t max_groups, hipStream_t stream);
void hipdf_gb_rowgid(const void* row_slot, const void* slot_gid, void* row_gid,
                     int64_t n, hipStream_t stream);
/* keys: device HipdfDenseKey[nkeys]. live: optional uint8 per dense id,
 * zeroed by the caller; every id some row lands on is set to 1. */
void hipdf_dense_gid(const void* keys, int nkeys, const void* sel,
                     void* row_gid, void* live, int64_t n,
                     hipStream_t stream);
/* table: int32[n] group ids of a dictionary's rows; a row where every one of
 * keys (device HipdfKeyCol[nkeys]) is NULL is moved to null_slot */
void hipdf_dense_null_slot(void* table, const void* keys, int nkeys,
                           int32_t null_slot, int64_t n, hipStream_t stream);
/* acc init for op: 0 sum 1 min 2 max 3 count */
void hipdf_gb_acc_init(int op, void* acc, int acc_is_double, int32_t ngroups,
                       hipStream_t stream);
/* acc: double or int64 [ngroups]; cnt: int64[ngroups], zeroed */
void hipdf_gb_agg(int op, int t, const void* vals, const void* vvalid,
                  const void* row_gid, void* acc, void* cnt, int acc_is_double,
                  int32_t ngroups, int64_t n, hipStream_t stream);
/* aggs: device HipdfAggDesc[naggs], accumulators [nrep * ngroups] */
void hipdf_gb_agg_multi(const void* aggs, int naggs, const void* row_gid,
                        const void* sel, int32_t ngroups, int nrep,
                        int64_t n, hipStream_t stream);
/* fold replicas 1..nrep-1 of acc / cnt into replica 0 */
void hipdf_gb_reduce_reps(int op, void* acc, int acc_is_double, void* cnt,
                          int32_t ngroups, int nrep, hipStream_t stream);
/* cnt: int64[n] -> validity words */
void hipdf_mask_from_nonzero(const void* cnt, void* mask, int64_t n,
                             hipStream_t stream);
/* hashes: int64[n]; regs: uint8 HyperLogLog registers, 2^p per group */
void hipdf_gb_hll(const void* hashes, const void* valid,
                  const void* row_gid, const void* sel, void* regs, int p,
                  int64_t n, hipStream_t stream);
/* vals: double, sorted within each group by perm (int32); starts and vcnt:
 * int64[ngroups]; out: double[ngroups] */
void hipdf_gb_percentile(const void* vals, const void* perm,
                         const void* starts, const void* vcnt, double p,
                         void* out, int ngroups, hipStream_t stream);
/* counts: int64[ngroups] of the valid rows */
void hipdf_gb_collect_count(const void* vvalid, const void* row_gid,
                            const void* sel, void* counts, int64_t n,
                            hipStream_t stream);
/* offsets and cursor: int64[ngroups] */
void hipdf_gb_collect_fill(int esize, const void* vals, const void* vvalid,
                           const void* row_gid, const void* sel,
                           const void* offsets, void* cursor, void* out,
                           int64_t n, hipStream_t stream);

/* ---- hash join (kernels/join.hip) -------------------------------------- */
/* chained table over the build side: head int32[cap], next int32[n];
 * hashes int32[n]; keys HipdfKeyCol[nkeys]; cap is a power of two */
void hipdf_join_build(const void* hashes, const void* keys, int nkeys,
                      void* head, void* next, int64_t cap, int64_t n,
                      hipStream_t stream);
/* how: 0 inner 1 left 2 semi 3 anti 4 full; counts: int64[n] */
void hipdf_join_count(int how, const void* lhashes, const void* lkeys,
                      const void* rkeys, int nkeys, const void* head,
                      const void* next, int64_t cap, void* counts, int64_t n,
                      hipStream_t stream);
/* lmap / rmap: int32 gather maps; right_matched: uint8 per build row or
 * NULL */
void hipdf_join_fill(int how, const void* lhashes, const void* lkeys,
                     const void* rkeys, int nkeys, const void* head,
                     const void* next, int64_t cap, const void* offsets,
                     void* lmap, void* rmap, void* right_matched, int64_t n,
                     hipStream_t stream);
int64_t join_probe_num_blocks(int64_t n);
/* dup_flag: int32[1], set when two build rows share a key */
void hipdf_join_check_unique(const void* keys, int nkeys, const void* next,
                             void* dup_flag, int64_t n, hipStream_t stream);
/* key_type >= 0: single integer key column of that HipdfType, hashed inline
 * (lkey / lvalid / rkey are its buffers; lhashes, lkeys, rkeys unused);
 * key_type < 0: precomputed lhashes + HipdfKeyCol descriptors.
 * match: int32[n]; block_counts: int64[join_probe_num_blocks(n)] */
void hipdf_join_probe_unique(int how, int key_type, const void* lkey,
                             const void* lvalid, const void* rkey,
                             const void* lhashes, const void* lkeys,
                             const void* rkeys, int nkeys, const void* head,
                             const void* next, int64_t cap, void* match,
                             void* right_matched, void* block_counts,
                             int64_t n, hipStream_t stream);
void hipdf_join_compact_unique(int how, const void* match,
                               const void* block_offsets, void* lmap,
                               void* rmap, int64_t n, hipStream_t stream);

/* ---- partition (kernels/partition.hip) --------------------------------- */
int64_t part_num_blocks(int64_t n);
/* part: int32[n]; counts: int64[nparts * part_num_blocks(n)] */
void hipdf_part_hist(const void* part, int nparts, void* counts, int64_t n,
                     hipStream_t stream);
void hipdf_part_scatter(const void* part, int nparts, const void* offsets,
                        void* perm, int64_t n, hipStream_t stream);

/* ---- sort (kernels/sort.hip) ------------------------------------------- */
int64_t sort_num_blocks(int64_t n);
int hipdf_sort_key_width(int t); /* value bytes of a HipdfType's sort key */
/* keys: uint64[n]; perm: int32[n] current order, or NULL for identity */
void hipdf_make_sort_keys(int t, const void* data, const void* valid,
                          const void* perm, int desc, int nulls_last,
                          int null_only, void* keys, int64_t n,
                          hipStream_t stream);
void hipdf_make_sort_keys_str(const void* offsets, const void* bytes,
                              const void* valid, const void* perm, int desc,
                              int chunk, void* keys, int64_t n,
                              hipStream_t stream);
void hipdf_make_sort_keys_i128(const void* data, const void* valid,
                               const void* perm, int desc, int word,
                               void* keys, int64_t n, hipStream_t stream);
/* counts: int64[256 * sort_num_blocks(n)], digit-major */
void hipdf_radix_count(const void* keys, int shift, void* counts, int64_t n,
                       hipStream_t stream);
void hipdf_radix_scatter(const void* keys_in, const void* perm_in, int shift,
                         const void* offsets, void* keys_out, void* perm_out,
                         int64_t n, hipStream_t stream);
/* The whole multi-key sort, enqueued on `stream` with no allocation and no
 * synchronise: for each key, least significant first, build the u64 keys
 * (and their varying-bits word), then run the digit passes. Caller-owned
 * scratch: keys_a/keys_b u64[n], perm_a/perm_b i32[n], counts and scanned
 * i64[256 * sort_num_blocks(n)], scan_scratch i64[scan_scratch_elems of
 * that], diff u64[1]. out_perm i32[n] receives the final permutation. */
void hipdf_sort_order(const HipdfSortKey* sort_keys, int nkeys, int64_t n,
                      void* keys_a, void* keys_b, void* perm_a, void* perm_b,
                      void* counts, void* scanned, void* scan_scratch,
                      void* diff_word, void* out_perm, hipStream_t stream);

/* ---- file-format decode (kernels/decode.hip) --------------------------- */
/* parquet DELTA_BINARY_PACKED -> int64[n] */
void hipdf_pq_delta_i64(const void* b, int64_t nbytes, int64_t n, void* out,
                        hipStream_t stream);
/* out: uint8[n] */
void hipdf_orc_bool_rle(const void* b, int64_t nbytes, int64_t n, void* out,
                        hipStream_t stream);
/* out: int64[n] */
void hipdf_orc_rle_v2(const void* b, int64_t nbytes, int64_t n,
                      int is_signed, void* out, hipStream_t stream);
/* parquet PLAIN BYTE_ARRAY writer: 4-byte length + bytes per value */
void hipdf_str_plain_encode(const void* offsets, const void* bytes,
                            const void* out_off, void* out_len, void* out,
                            int mode, int64_t n, hipStream_t stream);
/* starts: int32[n_values]; lens: int64[n_values]; error: int32[1] */
void hipdf_str_plain_offsets(const void* data, int64_t nbytes,
                             int64_t n_values, void* starts, void* lens,
                             void* error, hipStream_t stream);
/* out: int32[n_values] */
void hipdf_rle_hybrid_decode(const void* data, int64_t nbytes, int bit_width,
                             void* out, int64_t n_values, hipStream_t stream);
/* runs: int64[4 * nruns] records [kind | bit_width << 1, absolute source
 * offset from base, output offset, count]; out: int32[n] */
void hipdf_rle_expand(const void* base, const void* runs, int64_t nruns,
                      int bit_width, void* out, int64_t n,
                      hipStream_t stream);
/* descs: int64 stream descriptors; one block decodes one stream */
void hipdf_rle_hybrid_batch(const void* base, const void* descs,
                            int nstreams, void* out, hipStream_t stream);
void hipdf_scatter_fixed(int esize, const void* vals, const void* idx,
                         void* out, int64_t n, hipStream_t stream);
/* levels: int32[n]; mask bit = (level == max_level) */
void hipdf_levels_to_mask(const void* levels, int max_level, void* mask,
                          int64_t n, hipStream_t stream);

/* ---- CSV / JSON field parsers (kernels/csv.hip) ------------------------ */
/* row_start / row_end: int32[nrows] byte ranges. type selects the output:
 * out_i64, out_f64, or a string slice (out_ss int32 start, out_sl int64
 * length). valid: uint8[nrows]; unsupported: int32[1] */
void hipdf_json_field(const void* bytes, const void* row_start,
                      const void* row_end, const void* name, int name_len,
                      int type, void* out_i64, void* out_f64, void* out_ss,
                      void* out_sl, void* valid, void* unsupported,
                      int64_t nrows, hipStream_t stream);
/* out: uint8[n], 1 where bytes[i] == target */
void hipdf_byte_eq(const void* bytes, int target, void* out, int64_t n,
                   hipStream_t stream);
void hipdf_csv_parse(const void* bytes, const void* row_start,
                     const void* row_end, int delim, int field_idx, int type,
                     void* out_i64, void* out_f64, void* out_ss,
                     void* out_sl, void* valid, void* unsupported,
                     int64_t nrows, hipStream_t stream);

/* ---- get_json_object (kernels/json.hip) -------------------------------- */
/* offsets int32[n+1] / bytes: the string column; valid: its mask or 0.
 * steps: int32 triples [kind, a, b] per path step (kind 0 = key named
 * names[a .. a+b), 1 = array index a). mode 0 (size pass) parses every row
 * and writes out_len int64[n], src_start / src_len int32[n] (the matched
 * value's span in bytes) and state uint8[n]: 0 NULL, 1 value, 2 left to the
 * host. mode 1 (write pass) re-reads the span of each state == 1 row and
 * writes its out_len normalised bytes at out_bytes + out_off[i] (int64) */
void hipdf_json_path(const void* offsets, const void* bytes,
                     const void* valid, const void* steps, const void* names,
                     int nsteps, const void* out_off, void* out_len,
                     void* src_start, void* src_len, void* state,
                     void* out_bytes, int mode, int64_t n,
                     hipStream_t stream);
/* The size pass for npaths (1..8) paths over the same column in one parse
 * per row. steps holds every path's triples one after another; path k owns
 * step_cnt[k] of them from triple step_off[k] on (both int32[npaths], device
 * memory), and every key name indexes the one names blob. The outputs hold
 * npaths * n entries, path-major: entry k * n + i is what hipdf_json_path's
 * size pass gives row i for path k alone. The write pass is hipdf_json_path
 * mode 1 over those npaths * n entries. */
void hipdf_json_path_multi(const void* offsets, const void* bytes,
                           const void* valid, const void* steps,
                           const void* step_off, const void* step_cnt,
                           const void* names, int npaths, void* out_len,
                           void* src_start, void* src_len, void* state,
                           int64_t n, hipStream_t stream);

/* ---- strings (kernels/strings.hip) ------------------------------------- */
/* op: 0 eq 1 ne 2 lt 3 le 4 gt 5 ge; out: uint8[n] */
void hipdf_str_cmp(int op, const void* ao, const void* ab, const void* bo,
                   const void* bb, void* out, int64_t n, hipStream_t stream);
void hipdf_str_cmp_scalar(int op, const void* ao, const void* ab,
                          const void* pat, int plen, void* out, int64_t n,
                          hipStream_t stream);
/* mode: 0 contains 1 starts-with 2 ends-with */
void hipdf_str_find(int mode, const void* ao, const void* ab, const void* pat,
                    int plen, void* out, int64_t n, hipStream_t stream);
void hipdf_str_like(const void* ao, const void* ab, const void* pat, int plen,
                    void* out, int64_t n, hipStream_t stream);
/* fill_nb bytes / fill_cps codepoints of fill; width in codepoints */
void hipdf_str_pad(int left, const void* ao, const void* ab,
                   const void* fill, int32_t fill_nb, int32_t fill_cps,
                   int32_t width, const void* out_off, void* out_len,
                   void* out, int mode, int64_t n, hipStream_t stream);
/* out: int32[n] */
void hipdf_str_locate(const void* ao, const void* ab, const void* needle,
                      int32_t needle_nb, int32_t pos, void* out, int64_t n,
                      hipStream_t stream);
/* out: int32[n] codepoints */
void hipdf_str_length(const void* ao, const void* ab, void* out, int64_t n,
                      hipStream_t stream);
/* ASCII case map over the byte buffer */
void hipdf_str_case(int upper, const void* in, void* out, int64_t nbytes,
                    hipStream_t stream);
void hipdf_i64_to_str(const void* vals, const void* out_off, void* out_len,
                      void* out, int mode, int64_t n, hipStream_t stream);
/* cols: device HipdfStrColDesc[ncols] */
void hipdf_str_concat_ws(const void* cols, int ncols, const void* sep,
                         int seplen, const void* out_off, void* out_len,
                         void* out, int mode, int64_t n,
                         hipStream_t stream);
/* out: bytes, same offsets as the input */
void hipdf_str_initcap(const void* ao, const void* ab, void* out,
                       int64_t n, hipStream_t stream);
void hipdf_str_reverse(const void* ao, const void* ab, void* out, int64_t n,
                       hipStream_t stream);
/* counts: int64[n] parts per row */
void hipdf_str_split_count(const void* ao, const void* ab,
                           const void* delim, int dlen, void* counts,
                           int64_t n, hipStream_t stream);
/* part_off: int64[n] scan of counts; out_ss / out_sl: int32 byte start and
 * int64 length of every part */
void hipdf_str_split_fill(const void* ao, const void* ab, const void* delim,
                          int dlen, const void* part_off, const void* counts,
                          void* out_ss, void* out_sl, int64_t n,
                          hipStream_t stream);
/* bstart int32[n] / blen int64[n]: byte ranges into ab */
void hipdf_str_trim_ranges(int mode, const void* ao, const void* ab,
                           void* bstart, void* blen, int64_t n,
                           hipStream_t stream);
void hipdf_str_concat2(const void* ao, const void* ab, const void* bo,
                       const void* bb, const void* out_off, void* out_len,
                       void* out_bytes, int mode, int64_t n,
                       hipStream_t stream);
/* start / slen in codepoints, SQL substring semantics */
void hipdf_substr_ranges(const void* ao, const void* ab, int start, int slen,
                         void* bstart, void* blen, int64_t n,
                         hipStream_t stream);
void hipdf_substr_copy(const void* ab, const void* bstart, const void* blen,
                       const void* out_off, void* out_bytes, int64_t n,
                       hipStream_t stream);

/* ---- window (kernels/window.hip) --------------------------------------- */
/* level_ptrs: device int64[nlevels] sparse-table level pointers; a_idx /
 * b_idx: int32[n] inclusive frame bounds */
void hipdf_win_minmax(int is_double, const void* level_ptrs, int nlevels,
                      const void* a_idx, const void* b_idx, int is_min,
                      void* out, int64_t n, hipStream_t stream);
/* vals: double[n] order key; seg_start / seg_end: int32[n] partition */
void hipdf_range_bounds(const void* vals, const void* seg_start,
                        const void* seg_end, double lo, double hi,
                        int lo_unb, int hi_unb, void* a_idx, void* b_idx,
                        int64_t n, hipStream_t stream);
/* keys: HipdfKeyCol[nkeys]; out: uint8[n], 1 where row i differs from i-1 */
void hipdf_change_flags(const void* keys, int nkeys, void* out, int64_t n,
                        hipStream_t stream);
void hipdf_iota_i32(void* out, int64_t n, hipStream_t stream);
/* double in/out; sums: double[scan_num_blocks(n)] */
void hipdf_scan_block_f64(const void* in, void* out, void* sums, int64_t n,
                          hipStream_t stream);
void hipdf_scan_add_offsets_f64(void* out, const void* sums, int64_t n,
                                hipStream_t stream);

/* ---- decimal128 (kernels/decimal128.hip) ------------------------------- */
/* int128 values are (lo, hi) int64 pairs */
void hipdf_dec_mul_div_wide(int is_div, const void* a, const void* b,
                            const void* av, const void* bv, int a_is_128,
                            int b_is_128, void* out, void* ov,
                            int out_is_128, int shift, int out_prec,
                            int64_t n, hipStream_t stream);
void hipdf_i128_rescale(const void* in, const void* iv, void* out, void* ov,
                        int shift, int out_prec, int out_is_64, int64_t n,
                        hipStream_t stream);
void hipdf_dec64_mul_div(int is_div, const void* a, const void* b,
                         const void* av, const void* bv, void* out, void* ov,
                         int out_is_128, int shift, int out_prec, int64_t n,
                         hipStream_t stream);
void hipdf_i128_arith(int op, const void* a, const void* b, const void* av,
                      const void* bv, void* out, void* ov, int64_t n,
                      hipStream_t stream);
/* out: uint8[n] */
void hipdf_i128_cmp(int op, const void* a, const void* b, const void* av,
                    const void* bv, void* out, void* ov, int64_t n,
                    hipStream_t stream);
void hipdf_i64_to_i128(const void* in, void* out, int64_t n,
                       hipStream_t stream);
void hipdf_i128_to_f64(const void* in, void* out, int64_t n,
                       hipStream_t stream);
/* acc: int128[ngroups]; cnt: int64[ngroups] */
void hipdf_gb_sum_i128_lds(int in_is_64, const void* vals,
                           const void* vvalid, const void* row_gid,
                           const void* sel, void* acc, void* cnt,
                           int ngroups, int64_t n, hipStream_t stream);
void hipdf_gb_sum_i64_to_i128(const void* vals, const void* vvalid,
                              const void* row_gid, const void* sel, void* acc,
                              void* cnt, int64_t n, hipStream_t stream);
void hipdf_gb_sum_i128(const void* vals, const void* vvalid,
                       const void* row_gid, const void* sel, void* acc,
                       void* cnt, int64_t n, hipStream_t stream);

/* ---- regex (kernels/regex.hip) ----------------------------------------- */
/* prog: int32 compiled program of nops ops, classes: its uint8 character
 * class tables; out_start int32, out_len int64; overflow: int32[1] */
void hipdf_regex_extract(const void* prog, int nops, const void* classes,
                         const void* offsets, const void* bytes, int group,
                         void* out_start, void* out_len, void* overflow,
                         int64_t n, hipStream_t stream);
void hipdf_regex_extract_all(const void* prog, int nops,
                             const void* classes, const void* offsets,
                             const void* bytes, int group,
                             const void* part_off, void* counts,
                             void* out_ss, void* out_sl, int mode,
                             void* overflow, int64_t n, hipStream_t stream);
void hipdf_regex_replace(const void* prog, int nops, const void* classes,
                         const void* offsets, const void* bytes,
                         const void* repl_ops, int nrepl, const void* lit,
                         const void* out_off, void* out_len, void* out_bytes,
                         int mode, void* overflow, int64_t n,
                         hipStream_t stream);
/* out: uint8[n] */
void hipdf_regex_match(const void* prog, int nops, const void* classes,
                       const void* offsets, const void* bytes, void* out,
                       void* overflow, int64_t n, hipStream_t stream);

/* ---- exact string<->decimal casts (kernels/cast_str.hip) --------------- */
/* out_kind: 0 dec64 (int64), 1 dec128 (2xint64), 2..5 int8/16/32/64 */
void hipdf_str_to_dec(const void* ao, const void* ab, const void* av,
                      int out_kind, int out_scale, int out_prec, void* out,
                      void* ov, int64_t n, hipStream_t stream);
void hipdf_dec_to_str(const void* vals, int in_is_128, int scale,
                      const void* out_off, void* out_len, void* out,
                      int mode, int64_t n, hipStream_t stream);

/* ---- datetime (kernels/datetime.hip) ----------------------------------- */
/* ts: int64 microseconds; trans: int64[n_trans] transition instants, offs:
 * int32[n_trans] UTC offsets */
void hipdf_tz_convert(const void* ts, const void* trans, const void* offs,
                      int n_trans, int to_utc, void* out, int64_t n,
                      hipStream_t stream);
/* tokens: int32[ntok] pattern; out: n fixed-width records of `width` bytes */
void hipdf_date_format(const void* ts_us, const void* tokens, int ntok,
                       int width, void* out, int64_t n, hipStream_t stream);
void hipdf_ts_parse(const void* ao, const void* ab, const void* av,
                    const void* tokens, int ntok, int width, void* out,
                    void* ov, int64_t n, hipStream_t stream);

/* ---- lists: segmented ops inside the rows of a LIST column
 * (kernels/lists.hip) ---------------------------------------------------- */
/* t: HipdfType of the child, or 7 for a string child (data = bytes,
 * eoffs = the child's int32 offsets; eoffs is ignored otherwise).
 * offsets: the LIST's int32[n+1]; offsets[0] need not be 0. cvalid: child
 * validity words or NULL. perm: int32[offsets[n]-offsets[0]] of GLOBAL child
 * indices, entry (p - offsets[0]) for child position p. Order inside a list
 * is (null rank, sort key, original index). */
int hipdf_list_block_cap(void); /* longest list the block tier sorts */
/* rows of length <= w (w in 8/16/32/64): w lanes own one list; longer rows
 * are left untouched */
void hipdf_list_sort_wave(int t, const void* data, const void* eoffs,
                          const void* cvalid, const void* offsets, int w,
                          int nulls_first, int desc, void* perm, int64_t n,
                          hipStream_t stream);
/* one block per listed row (int32 rows[nrows], each of length
 * <= hipdf_list_block_cap()) */
void hipdf_list_sort_block(int t, const void* data, const void* eoffs,
                           const void* cvalid, const void* offsets,
                           const void* rows, int64_t nrows, int nulls_first,
                           int desc, void* perm, hipStream_t stream);
/* perm from an ascending sort; keep: uint8[total], 1 = first occurrence */
void hipdf_list_distinct_flags(int t, const void* data, const void* eoffs,
                               const void* cvalid, const void* offsets,
                               int64_t n, const void* perm, void* keep,
                               int64_t total, hipStream_t stream);
/* out: int32[n] global child index of the first min (max) non-null element,
 * -1 for a null (rvalid), empty or all-null list */
void hipdf_list_argminmax(int t, const void* data, const void* eoffs,
                          const void* cvalid, const void* offsets,
                          const void* rvalid, int w, int is_max, void* out,
                          int64_t n, hipStream_t stream);
/* Two-list set operations: side a is probed against side b row by row; both
 * are LISTs of n rows with the same element type t, each with its own child,
 * validity and first offset. bperm is b's ascending, nulls-first sort
 * permutation (hipdf_list_sort_*), or NULL when b has no elements.
 * member: uint8[total], total = aoffsets[n] - aoffsets[0]; entry p is 1 when
 * element aoffsets[0] + p of a equals an element of the same row of b (null
 * equals null, NaN equals NaN, -0.0 equals 0.0) */
void hipdf_list_member_flags(int t, const void* adata, const void* aeoffs,
                             const void* acvalid, const void* aoffsets,
                             const void* bdata, const void* beoffs,
                             const void* bcvalid, const void* boffsets,
                             const void* bperm, int64_t n, void* member,
                             int64_t total, hipStream_t stream);
/* arrays_overlap from a's member flags, w lanes (8/16/32/64) per row. out:
 * uint8[n], 1 = a non-null element is shared. vout: validity words covering
 * n rows, every word written whole; a row is NULL when either row validity
 * (arvalid / brvalid, may be NULL) says so, or when nothing is shared, both
 * rows are non-empty and either holds a null element */
void hipdf_list_overlap(const void* member, const void* aoffsets,
                        const void* acvalid, const void* arvalid,
                        const void* boffsets, const void* bcvalid,
                        const void* brvalid, const void* bperm, int w,
                        void* out, void* vout, int64_t n,
                        hipStream_t stream);
/* array_union's gather map. ascan: int64[atotal + 1] exclusive scan of a's
 * kept flags (last slot = kept count), bscan likewise. new_offs: int32[n+1];
 * idx: int32[kept a + kept b] rows of concat(a.child, b.child), b's child
 * starting at row bbase; result row r = a's kept elements, then b's */
void hipdf_list_union_map(const void* ascan, const void* aoffsets,
                          int64_t atotal, const void* bscan,
                          const void* boffsets, int64_t btotal, int64_t n,
                          int64_t bbase, void* new_offs, void* idx,
                          hipStream_t stream);
/* Element to row map of a LIST of n rows, total = offsets[n] - offsets[0]
 * elements, one thread per element. rowid: int32[total], the row that owns
 * element offsets[0] + p; pos: int32[total], its 0-based place in that row,
 * or NULL when not wanted. Both are indexed from 0 */
void hipdf_list_elem_rows(const void* offsets, int64_t n, void* rowid,
                          void* pos, int64_t total, hipStream_t stream);
/* exists (mode 0) / forall (mode 1) over pred, a BOOL column with one entry
 * per element from offsets[0] (pvalid may be NULL), w lanes (8/16/32/64) per
 * row. out: uint8[n]; vout: validity words covering n rows, every word
 * written whole. exists: 1 when a predicate is true, else NULL when one is
 * null, else 0. forall: 0 when a predicate is false, else NULL when one is
 * null, else 1. A row that rvalid (may be NULL) marks null is NULL */
void hipdf_list_bool_reduce(const void* pred, const void* pvalid,
                            const void* offsets, const void* rvalid, int w,
                            int mode, void* out, void* vout, int64_t n,
                            hipStream_t stream);
/* Per-row search of a LIST of n rows for the row's own needle, w lanes
 * (8/16/32/64) per row. t / data / eoffs / cvalid / offsets / rvalid describe
 * the list as above; ndata / neoffs / nvalid are a column of the element type
 * with one needle per row (nvalid may be NULL). A row is live when it and its
 * needle are non-null; other rows are not read through. An element matches
 * when it is non-null and equals the needle (NaN equals NaN, -0.0 equals 0.0,
 * strings by bytes). Each output may be NULL when not wanted.
 * match: uint8[offsets[n] - offsets[0]], 1 at a match, 0 all over a row that
 * is not live; first: int64[n], 1-based place of the first match, 0 for none;
 * vout: validity words covering n rows, every word written whole, bit = live */
void hipdf_list_find(int t, const void* data, const void* eoffs,
                     const void* cvalid, const void* offsets,
                     const void* rvalid, const void* ndata,
                     const void* neoffs, const void* nvalid, int w,
                     void* match, void* first, void* vout, int64_t n,
                     hipStream_t stream);
/* slice(list, start, length) per row; start and length are int32[n] columns
 * with their validity (each may be NULL). A row is live when all three are
 * non-null. start is 1-based, a negative start counts from the end, a first
 * element outside the row gives an empty result; the arithmetic is 64-bit.
 * src_start: int32[n], global child index of the first element taken;
 * out_len: int64[n + 1], elements taken (0 for a row that is not live or is
 * in error), entry n is 0; vout: validity words covering n rows, bit = live;
 * err: uint64[2], zeroed by the caller: live rows with start == 0, live rows
 * with length < 0 are added to it */
void hipdf_list_slice_ranges(const void* offsets, const void* rvalid,
                             const void* start, const void* svalid,
                             const void* length, const void* lvalid,
                             void* src_start, void* out_len, void* vout,
                             void* err, int64_t n, hipStream_t stream);
/* gather map of slice, one thread per output element: new_offs int32[n + 1]
 * from 0 to total; idx[p] = src_start[row] + (p - new_offs[row]) */
void hipdf_list_slice_map(const void* new_offs, const void* src_start,
                          int64_t n, void* idx, int64_t total,
                          hipStream_t stream);

/* ---- array builders: array(), concat, flatten, sequence, array_join ---- */
/* Up to 8 per-row operands of one launch. Unlike the descriptor structs
 * above this one is read from HOST memory by the entry point and handed to
 * the kernel by value; more operands take more launches. Unused slots are
 * NULL. a[j]: operand j's values (list_interleave) or int32 offsets[n + 1]
 * (list_concat_*); valid[j]: its validity words or NULL. */
#define HIPDF_LIST_MAX_OPERANDS 8
typedef struct {
  const void* a[HIPDF_LIST_MAX_OPERANDS];
  const void* valid[HIPDF_LIST_MAX_OPERANDS];
} HipdfListOperands;
HIPDF_STATIC_ASSERT(sizeof(HipdfListOperands) == 128, "packed as <16q");
/* array(c_0 .. c_{k-1}) over fixed-width operands of esize (1/2/4/8) bytes,
 * n rows each, n * k <= INT32_MAX: out[i * k + j] = c_j[i]. ops (host) holds
 * operands j0 .. j0 + kk - 1 of the k. vout: validity words covering n * k
 * elements, or NULL when no operand has a mask. shared == 0: every operand
 * is in this launch and each word is stored whole; shared == 1: the caller
 * has zeroed vout and the launches OR their bits in. new_offs: int32[n + 1],
 * i * k, or NULL. */
void hipdf_list_interleave(int esize, const void* ops, int k, int j0, int kk,
                           int shared, void* out, void* vout, void* new_offs,
                           int64_t n, hipStream_t stream);
/* the same layout as a gather map over the concatenation of the k operand
 * columns: idx[i * k + j] = j * n + i (int32[n * k]); new_offs as above */
void hipdf_list_interleave_map(int k, void* idx, void* new_offs, int64_t n,
                               hipStream_t stream);
/* concat of k LIST columns, row lengths. Launches go over the operands in
 * order, kk (<= 8) at a time, first / last marking the outer ones. out_len:
 * int64[n + 1], the running and after the last launch the final length, 0
 * for a row that is null in any operand, entry n is 0; prefix: int32[n] or
 * NULL, the running length before this launch's operands; vout: validity
 * words covering n rows, the AND of the operands' */
void hipdf_list_concat_lens(const void* ops, int kk, int first, int last,
                            void* out_len, void* prefix, void* vout,
                            int64_t n, hipStream_t stream);
/* concat's gather map for the operands of one launch: new_offs int32[n + 1]
 * from 0 to total; prefix as written by list_concat_lens for the same
 * operands (NULL for the first launch); cbase (host): int64[kk], row of the
 * concatenated children at which each operand's child begins. Writes
 * idx[p] (int32[total]) for the elements that come from these operands. */
void hipdf_list_concat_map(const void* ops, const void* cbase, int kk,
                           const void* new_offs, const void* prefix,
                           int64_t n, void* idx, int64_t total,
                           hipStream_t stream);
/* flatten(LIST<LIST<T>>), n >= 1 rows, w lanes (8/16/32/64) per row. outer /
 * rvalid: the outer offsets and validity; inner / ivalid: the inner LIST
 * column's. new_offs: int32[n + 1] = inner[outer[i]] - inner[outer[0]];
 * vout: validity words covering n rows, bit = outer row valid and no inner
 * array of the row null; span: int64[2] = inner[outer[0]], inner[outer[n]] */
void hipdf_list_flatten(const void* outer, const void* rvalid,
                        const void* inner, const void* ivalid, int w,
                        void* new_offs, void* vout, void* span, int64_t n,
                        hipStream_t stream);
/* sequence(start, stop[, step]) per row, t = HIPDF_I32 or HIPDF_I64 for all
 * three; step == NULL stands for 1 where start <= stop, else -1. out_len:
 * int64[n + 1] elements per row (1 + (stop - start) / step, capped at 2^31),
 * 0 for a null or an illegal row, entry n is 0; vout: validity words
 * covering n rows; err: int64[4], err[0] preset to INT64_MAX: the least
 * illegal row (start != stop and step == 0 or pointing away from stop) and
 * its start, stop and step */
void hipdf_sequence_ranges(int t, const void* start, const void* avalid,
                           const void* stop, const void* bvalid,
                           const void* step, const void* svalid,
                           void* out_len, void* vout, void* err, int64_t n,
                           hipStream_t stream);
/* out[p] = start[row] + (p - offs[row]) * step[row]; offs int32[n + 1] from
 * 0 to total */
void hipdf_sequence_fill(int t, const void* offs, const void* start,
                         const void* stop, const void* step, int64_t n,
                         void* out, int64_t total, hipStream_t stream);
/* array_join(LIST<STRING>, delimiter[, replacement]) in three passes around
 * two scans. offsets / rvalid: the list; eoffs / bytes / cvalid: its string
 * child; total = offsets[n] - offsets[0]; dlen: delimiter bytes; rlen:
 * replacement bytes, -1 for none (null elements are skipped).
 * sizes: contrib int64[total + 1], bytes each element adds with its
 * delimiter, entry total is 0. rows: out_len int64[n + 1] from the exclusive
 * scan of contrib. write: out_off is the exclusive scan of out_len. */
void hipdf_array_join_sizes(const void* offsets, const void* rvalid,
                            const void* eoffs, const void* cvalid, int dlen,
                            int rlen, int64_t n, void* contrib, int64_t total,
                            hipStream_t stream);
void hipdf_array_join_rows(const void* offsets, const void* scanned, int dlen,
                           int64_t n, void* out_len, hipStream_t stream);
void hipdf_array_join_write(const void* offsets, const void* rvalid,
                            const void* eoffs, const void* bytes,
                            const void* cvalid, const void* delim, int dlen,
                            const void* repl, int rlen, const void* scanned,
                            const void* out_off, int64_t n, void* out,
                            int64_t total, hipStream_t stream);

/* ---- native in-order scan reader (scan_reader.hip) --------------------- */
/* Host-only walk of one parquet column chunk: one (value offset from the
 * chunk start, value bytes, values) int64 triple per data page into out
 * (room for max_out triples). Returns the number of pages, or a negative
 * code when the chunk is not eligible: eligible is uncompressed, no
 * dictionary page, every data page (v1 or v2) PLAIN with phys_width 4 or 8
 * bytes per value, and max_def == 0 or every page's definition levels plain
 * RLE runs of max_def. Never reads at or beyond chunk + nbytes. */
int64_t hipdf_pq_plain_pieces(const void* chunk, int64_t nbytes,
                              int64_t num_values, int max_def, int phys_width,
                              int64_t* out, int64_t max_out);

/* one column chunk of a scan submit; the array stays in host memory */
typedef struct {
  const void* src;     /* host: first byte of the chunk in the file mapping */
  int64_t nbytes;      /* chunk length */
  int32_t phys_width;  /* 4 or 8 */
  int32_t dst_width;   /* phys_width, or 8 over 4: signed widen */
  void* dst;           /* device: where the chunk's first value lands */
  int64_t num_values;
  int32_t group;       /* hand-over unit (file index), 0 .. n_groups-1 */
  int32_t max_def;
  /* device: the destination column's LSB-first validity mask, zeroed before
   * the submit, or NULL. NULL: the chunk must be all valid (the rule and the
   * error codes of hipdf_pq_plain_pieces). Not NULL: max_def must be 1, the
   * chunk may hold nulls, null rows of dst are written as zero and bit
   * valid_bit0 + i of the mask is set when row i of the chunk is valid. */
  void* valid;
  int64_t valid_bit0;  /* bit of the chunk's first row; any offset */
} HipdfScanChunk;
HIPDF_STATIC_ASSERT(sizeof(HipdfScanChunk) == 64, "packed as <qqiiqqiiqq");

typedef struct HipdfScanReader HipdfScanReader;
/* at most 8 worker threads, each with a scratch buffer of piece_bytes (and
 * the mask words and tile counts of a nullable slice of that many bytes);
 * n_streams <= n_threads copy streams. NULL on failure. */
HipdfScanReader* hipdf_scan_open(int n_threads, int n_streams,
                                 int64_t piece_bytes);
/* Walks every chunk, cuts it into pieces of at most piece_bytes and queues
 * them group-major. Every dst buffer must be allocated before the call (see
 * the memory rule in scan_reader.hip); an event recorded on `consumer` gates
 * the first write. Returns a ticket (> 0), or a negative code and nothing
 * queued: a hipdf_pq_plain_pieces code when a chunk is not eligible. The
 * definition levels of a chunk with a validity mask are decoded later, on the
 * worker threads; a page whose levels are malformed or disagree with its
 * value bytes fails the submit, which hipdf_scan_wait_group reports. */
int64_t hipdf_scan_submit(HipdfScanReader* r, const HipdfScanChunk* chunks,
                          int64_t n_chunks, int n_groups,
                          hipStream_t consumer);
/* Blocks the calling thread until every piece of `group` is enqueued, then
 * makes `consumer` wait for them on the device. 0, or negative on a copy
 * error / a cancelled submit. */
int hipdf_scan_wait_group(HipdfScanReader* r, int64_t ticket, int group,
                          hipStream_t consumer);
/* Ends a submit, finished or not: claims no further piece, waits for what
 * is claimed to be enqueued and, when a group with copies was never waited
 * for, for the copies themselves. Every ticket must be cancelled once. */
void hipdf_scan_cancel(HipdfScanReader* r, int64_t ticket);
/* cancels what is left, joins the workers, frees streams and scratch */
void hipdf_scan_close(HipdfScanReader* r);

/* ---- device memory pool (pool.hip) ------------------------------------- */
/* reserve `bytes` (or fraction of free memory if bytes==0) as the pool
 * slab; returns 0 on success */
int hipdf_pool_init(double fraction, size_t bytes);
int hipdf_pool_active(void);
/* failure callback: returns nonzero if it freed memory and the alloc
 * should be retried (Python side: spill device->host) */
typedef int (*hipdf_failure_cb)(size_t needed, int retry);
void hipdf_pool_set_failure_cb(hipdf_failure_cb cb);
size_t hipdf_pool_used(void);           /* slab bytes in use + overflow */
size_t hipdf_pool_reserved(void);       /* slab capacity */
size_t hipdf_pool_high_watermark(void); /* peak slab bytes in use */
size_t hipdf_pool_overflow(void);       /* bytes served outside the slab */
void* hipdf_pool_alloc(size_t n);
void hipdf_pool_free(void* p);
/* torch CUDAPluggableAllocator entry points */
void* hipdf_torch_malloc(size_t size, int device, hipStream_t stream);
void hipdf_torch_free(void* ptr, size_t size, int device,
                      hipStream_t stream);
/* host-memory selftest of the arena logic; returns 0 on success, a nonzero
 * step id on the first failed invariant */
int hipdf_pool_selftest(void);

#ifdef __cplusplus
}
#endif
#undef HIPDF_STATIC_ASSERT

#endif /* HIPDF_H */
