/*
 * nrtgpu.h -- C ABI of the MI355X-native query-execution path for nrtsearch.
 *
 * This is the drop-in boundary: everything nrtsearch does below
 *   searcher.search(query, collectorManager)
 *     src/main/java/com/yelp/nrtsearch/server/handler/SearchHandler.java:1412-1413 (single query)
 *     src/main/java/com/yelp/nrtsearch/server/handler/SearchHandler.java:556        (per retriever)
 * for an eligible query (pure-SHOULD BooleanQuery of TermQuery clauses / single TermQuery under
 * the default BM25Similarity, or an exact float vector query) is replaced by calls into this
 * library.  The reference has no native boundary of its own (pure JVM); the JNI / FFM stub a
 * maintainer adds on the Java side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns NRTGPU_OK (0) or a negative nrtgpu_status; nrtgpu_last_error()
 *    returns a thread-local UTF-8 message for the last failure on the calling thread.
 *  - thread-safety: any number of host threads may call the search / knn / rescore functions
 *    concurrently on one ctx (SEARCH-pool threads, src/main/java/com/yelp/nrtsearch/server/
 *    concurrent/ExecutorFactory.java:80-117).  Segment lifecycle calls for one nrtgpu_seg must not
 *    race with each other; releasing a segment that a running search uses is undefined.
 *  - ownership: input pointers are borrowed for the duration of the call; outputs are written
 *    into caller-allocated arrays of the stated capacity.  No callbacks into the caller.
 *  - plain C types only: no torch / HIP types cross this boundary.
 *  - there is NO CPU fallback inside the library: with no usable gfx950 device nrtgpu_create
 *    fails with NRTGPU_ERR_HIP; NRTGPU_ERR_UNSUPPORTED tells the caller to run its own
 *    (Lucene) path for that query.
 */
#ifndef NRTGPU_H
#define NRTGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  NRTGPU_OK = 0,
  NRTGPU_ERR_INVALID_ARG = -1, /* IllegalArgumentException in the reference (e.g. numHits <= 0) */
  NRTGPU_ERR_HIP = -2,         /* device / runtime failure -> IOException -> gRPC INTERNAL */
  NRTGPU_ERR_OOM = -3,
  NRTGPU_ERR_UNSUPPORTED = -4, /* shape not handled on device: caller falls back to Lucene */
  NRTGPU_ERR_STATE = -5,       /* lifecycle misuse (e.g. search on an unsealed segment) */
  NRTGPU_ERR_TIMEOUT = -6      /* the calling thread's deadline passed before the work was launched (nrtgpu_set_thread_deadline_ns):
                                * gRPC DEADLINE_EXCEEDED / SearchResponse.hitTimeout */
} nrtgpu_status;

typedef struct nrtgpu_ctx nrtgpu_ctx;
typedef struct nrtgpu_seg nrtgpu_seg;

/* Limits of the device fast path (queries outside them get NRTGPU_ERR_UNSUPPORTED). */
#define NRTGPU_MAX_K 1024          /* numHits handled by the LDS top-k */
#define NRTGPU_MAX_TERMS 32        /* SHOULD clauses per query */
#define NRTGPU_MAX_MASKS 8         /* FILTER (and, separately, MUST_NOT) clauses per query */
#define NRTGPU_TILE_DOCS 1024      /* docs per wave-private LDS accumulator sub-tile */

typedef struct {
  int32_t device_id;        /* HIP device ordinal this ctx owns (one process per GPU) */
  int32_t max_batch;        /* max queries per batch call; 0 => 1024 */
  int32_t target_items;     /* work items (query x doc-range) aimed for per batch; 0 => auto */
  int32_t collect_timing;   /* !=0: bracket the scan kernel with HIP events (nrtgpu_get_stats) */
  int32_t flags;            /* NRTGPU_FLAG_* */
  int32_t host_threads;     /* planner threads used inside one batch call (term-dictionary lookups); 0 => 4 */
  int32_t lookup_budget_pct; /* HBM a segment may spend on doc -> posting lookup structures of the dynamic-pruning route (per term a
                             * 16-bit code map or lookup cells), in percent of its resident posting bytes, granted to the largest
                             * terms first; 0 => 150; < 0 => none (every lookup is a binary search in the postings: slower, same
                             * results) */
  int32_t reserved;
} nrtgpu_config;

#define NRTGPU_FLAG_NO_PREFETCH 1     /* scan kernel without the one-tile-ahead posting prefetch (A/B) */
#define NRTGPU_FLAG_NO_FIXED_POINT 2  /* always accumulate in fp64 (A/B; results are identical either way) */
#define NRTGPU_FLAG_NO_LIVE_FOLD 8     /* A/B: liveDocs stay a mask read by the scan instead of being folded into the posting columns */
#define NRTGPU_FLAG_NO_MASK_VARIANT 4   /* A/B: docs outside liveDocs / a mask are checked one by one (general sweep) */
#define NRTGPU_FLAG_PACKED_POSTINGS 32  /* compressed postings: every segment of this context keeps ONE 32-bit word per
                                        * posting in HBM (20-bit doc offset inside its 2^20-doc super-window | 12-bit score code) instead of
                                        * a docid and a code column: half the posting bytes, same results bit for bit.  liveDocs are then not
                                        * folded into the postings (the scorers test the mask).  Postings the 12-bit code cannot name (freq > 12
                                        * or norm byte >= 128) go through a per-upload-group exception list (4 B each).  A separately
                                        * reported configuration (its own roofline denominator). */
#define NRTGPU_FLAG_BLOCKING_WAIT 64    /* callers sleep until their results are there instead of spinning on the stream: for deployments
                                        * where several processes (one per GPU) with several calls in flight each share the host's CPUs.
                                        * Costs a wake-up (tens of microseconds) per call */
#define NRTGPU_FLAG_NO_VECTOR_SKETCH 128 /* vector fields keep no fp16 copy of their rows (+50 % of the fp32 matrix, built by a field's first exact search): the exact search then
                                         * nominates from the fp32 rows (2x the bytes per pass, 32 queries per pass instead of 64).
                                         * Results are the same bits either way */
#define NRTGPU_FLAG_NO_PRUNE 16        /* never take the MaxScore route: every query is scanned exhaustively and total_hits is
                                        * always the exact count (the relation still follows totalHitsThreshold) */

const char* nrtgpu_version(void);
const char* nrtgpu_last_error(void);

int  nrtgpu_create(const nrtgpu_config* cfg, nrtgpu_ctx** out);
void nrtgpu_destroy(nrtgpu_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * Segment store: a read-only columnar replica of one immutable Lucene segment's scoring data,
 * filled through Lucene's public reader APIs at searcher-refresh / warm time
 * (hook: ShardSearcherFactory.newSearcher, src/main/java/com/yelp/nrtsearch/server/index/
 * ShardState.java:506-527; keyed by the segment core CacheKey on the Java side).
 * --------------------------------------------------------------------------------------------- */
int  nrtgpu_segment_begin(nrtgpu_ctx* ctx, int32_t max_doc, int32_t device_hint, nrtgpu_seg** out);
/* norms of one field: leaf.getNormValues(field) as bytes (SmallFloat.intToByte4 of the field
 * length); NULL => norms omitted, norm value 1 for every doc (AtomFieldDef.java:123-126). */
int  nrtgpu_segment_add_field_norms(nrtgpu_seg* seg, int32_t field_id, const uint8_t* norm_bytes);
/* postings of n_terms terms of one field: TermsEnum/PostingsEnum flattened column-major.
 * term_hash identifies a term (any injective 64-bit id chosen by the caller); offsets has
 * n_terms+1 entries into docids/freqs; docids ascending within a term; freqs NULL => all 1
 * (IndexOptions.DOCS).  May be called several times per segment/field. */
int  nrtgpu_segment_add_terms(nrtgpu_seg* seg, int32_t field_id, int64_t n_terms, const int64_t* term_hash,
                              const int64_t* offsets, const int32_t* docids, const int32_t* freqs);
/* float vectors of one field (leaf.getFloatVectorValues): n rows of `dim` fp32, row-major;
 * ord_to_doc NULL => ordinal == docid (dense).  Any dim <= 2048 (more: NRTGPU_ERR_UNSUPPORTED, the field stays on the
 * caller's path): rows are kept zero-padded to a multiple of 16 elements and query vectors are padded alike inside the
 * search calls -- zeros add nothing to a dot product, a squared norm or a squared distance, so scores are the field's own
 * (the reference's vector tests run at dim = 3: VectorFieldDefTest.java:1885-1965).  Queries pass the field's dim. */
int  nrtgpu_segment_add_vectors(nrtgpu_seg* seg, int32_t field_id, int32_t dim, int32_t n,
                                const int32_t* ord_to_doc, const float* row_major);
/* byte vectors of one field (leaf.getByteVectorValues; VECTOR_ELEMENT_BYTE fields, VectorFieldDef.java:677-882): n rows of `dim`
 * int8, row-major; ord_to_doc as nrtgpu_segment_add_vectors.  dim <= 2048 (more: NRTGPU_ERR_UNSUPPORTED).  Rows are kept
 * zero-padded to whole 64-element steps of the i8 matrix instruction, in its operand order -- up to 8 steps (512 elements) as
 * many as the dimension needs, beyond that the next step count with a divisor in 4..8 (9 -> 10, 11 -> 12, 13 -> 14, 17 -> 18,
 * 19 -> 20, 22 and 23 -> 24, 26 and 27 -> 28, 29 -> 30, 31 -> 32: up to 11 % more bytes, for dimensions 513-576) -- with |v|^2
 * per row (int32) computed on the device at upload; queries pass the field's dim.  A field holds float rows or byte rows, never both (the second kind:
 * NRTGPU_ERR_INVALID_ARG). */
int  nrtgpu_segment_add_byte_vectors(nrtgpu_seg* seg, int32_t field_id, int32_t dim, int32_t n,
                                     const int32_t* ord_to_doc, const int8_t* row_major);
/* A per-doc value column of one field: ONE 32-bit value per doc (IntFieldDef / FloatFieldDef doc values; for a multi-valued
 * field the caller uploads the selector's pick -- SortedNumericSelector MIN / MAX, src/main/java/com/yelp/nrtsearch/server/field/
 * properties/Sortable.java:34-45 -- as a column of its own field id).  docs: the n docs that have a value, ascending leaf docids
 * (NULL: doc i = i, n == max_doc); values: n x 4 bytes of the kind.  Docs not listed have no value.  The column is independent of
 * whatever else the field id holds (postings, norms); before the seal only (after: NRTGPU_ERR_STATE); forks share it;
 * nrtgpu_segment_device_bytes counts it.  Resident as one order-preserving 32-bit code per doc plus one bit per doc where some
 * doc lacks a value.  Sorting is its first reader (nrtgpu_search_sorted_batch).  NRTGPU_ERR_INVALID_ARG: kind out of range,
 * n < 0 or n > max_doc, docs not strictly ascending or outside [0, max_doc), docs == NULL with n != max_doc, values == NULL with
 * n > 0, a second column on the field -- of either arity: a field that holds a multi-valued column
 * (nrtgpu_segment_add_doc_values_multi) takes no single-valued one.  64-bit values are nrtgpu_segment_add_doc_values64's.  Out of
 * scope: updatable doc values. */
#define NRTGPU_DOCVALUES_INT32 0    /* IntFieldDef: SortField.Type.INT */
#define NRTGPU_DOCVALUES_FLOAT32 1  /* FloatFieldDef: SortField.Type.FLOAT */
int  nrtgpu_segment_add_doc_values(nrtgpu_seg* seg, int32_t field_id, int32_t kind, int32_t n, const int32_t* docs,
                                   const void* values);
/* A MULTI-VALUED value column of one field: any number of 32-bit values per doc -- every value of a SORTED_NUMERIC int / float
 * field (src/main/java/com/yelp/nrtsearch/server/field/IntFieldDef.java:62-70,83-85 through LoadedDocValues.SortedIntegers,
 * doc/LoadedDocValues.java:483-500; floats :600-603), or the global ordinals of a SORTED_SET string field as INT32 values
 * (search/collectors/additional/OrdinalTermsCollectorManager.java:189-226).  value_docs[i] is the leaf docid of value i,
 * NON-DECREASING and in [0, max_doc); values: n_values x 4 bytes of the kind.  A doc that is not listed has no value, a doc
 * listed c times has c values; duplicates inside a doc are kept and count each (docValueCount()).  n_values == 0 is a valid
 * column: the kind is known and no doc has a value, which differs from "the leaf lacks the column".  No limit on values per doc.
 * Readers: the terms counts (every value instance of a hit adds 1) and the range clauses of the doc-set requests (a doc passes
 * iff SOME value is in the range); a sort refuses such a column (it names ONE value per doc: upload the selector's pick
 * single-valued, above).  Resident as uint32 start[]: one entry per doc, padded to whole sub-tiles, plus one -- doc d's values
 * are codes[start[d] .. start[d + 1]), every padding entry equals n_values -- and uint32 codes[]: the values' order-preserving
 * codes in upload order.  Before the seal only (after: NRTGPU_ERR_STATE); forks share it; nrtgpu_segment_device_bytes counts it.
 * NRTGPU_ERR_INVALID_ARG: seg NULL, kind out of range, n_values < 0, a NULL array with n_values > 0, value_docs decreasing or
 * outside [0, max_doc), a second column of either arity on the field. */
int  nrtgpu_segment_add_doc_values_multi(nrtgpu_seg* seg, int32_t field_id, int32_t kind, int32_t n_values,
                                         const int32_t* value_docs, const void* values);
/* A per-doc value column of 64-BIT values: LongFieldDef, DateTimeFieldDef (epoch milliseconds) and DoubleFieldDef doc values,
 * which the reference sorts as SortField.Type.LONG / DOUBLE (src/main/java/com/yelp/nrtsearch/server/field/DateTimeFieldDef.java:
 * 108-125, LongFieldDef.java:103-105, DoubleFieldDef.java:105-107) and filters with SortedNumericDocValuesField.newSlowRangeQuery
 * over 64-bit values (LongFieldDef.java:124-154, DateTimeFieldDef.java:133-167).  nrtgpu_segment_add_doc_values' contract, word
 * for word, with values of n x 8 bytes: the column is single-valued (the selector's pick for a multi-valued field); docs strictly
 * ascending, or NULL with n == max_doc; before the seal only (after: NRTGPU_ERR_STATE); forks share it;
 * nrtgpu_segment_device_bytes counts it; a field holds ONE column of any width or arity (a second one: NRTGPU_ERR_INVALID_ARG,
 * like every other argument error listed there; kind outside 2..3 is one).  Resident as one order-preserving uint64 code per doc,
 * padded to whole sub-tiles, plus the `has` words where some doc lacks a value; the least and the greatest code of the column
 * stay on the segment (a column with n == 0 has none): the window a sort packs its keys in.  Codes compare like Long.compare /
 * Double.compare: -0.0 < +0.0, every NaN the canonical 0x7FF8000000000000 and above +inf.
 * Readers: nrtgpu_search_sorted64_batch, nrtgpu_search_docset_sorted64_batch, nrtgpu_segment_set_mask_from_values64,
 * nrtgpu_count_ranges_batch, nrtgpu_count_terms64_batch, nrtgpu_count_docset_terms64_batch.  The 32-bit
 * entries (nrtgpu_search_sorted_batch, nrtgpu_count_terms_batch, the doc-set entries' sort, count and range clauses,
 * nrtgpu_segment_set_mask_from_values) refuse a field that holds a 64-bit column with NRTGPU_ERR_UNSUPPORTED, the reason naming
 * the 64-bit entry (terms counts: 64-bit buckets are not built by the 32-bit entries, nrtgpu_count_terms64_batch /
 * nrtgpu_count_docset_terms64_batch build them); the 64-bit entries refuse a 32-bit or multi-valued column the
 * same way.  Neither reads a column at the other width.  Out of scope: multi-valued 64-bit columns, doc-set
 * range CLAUSES over 64-bit columns (a range over one is a built mask), updatable doc values. */
#define NRTGPU_DOCVALUES_INT64   2  /* LongFieldDef, DateTimeFieldDef (epoch millis): SortField.Type.LONG */
#define NRTGPU_DOCVALUES_FLOAT64 3  /* DoubleFieldDef: SortField.Type.DOUBLE */
int  nrtgpu_segment_add_doc_values64(nrtgpu_seg* seg, int32_t field_id, int32_t kind, int32_t n, const int32_t* docs,
                                     const void* values /* n x 8 bytes */);
/* builds the per-term doc-range tables; the segment becomes searchable */
int  nrtgpu_segment_seal(nrtgpu_seg* seg);
/* leaf.getLiveDocs() as 64-bit words, bit d set = doc d live; NULL => all live.  May be called
 * again after seal (only liveDocs change between reader versions of one segment).  Costs one device
 * pass over the segment's postings: the postings of deleted docs are re-coded to score the neutral
 * element, so searches pay nothing per query for deletes.  Thread-safe against searches: the call waits for
 * the searches running over this segment and later ones wait for it (they see the new liveDocs; one
 * liveDocs version per segment handle at a time).  Bits at or beyond max_doc are ignored. */
int  nrtgpu_segment_set_live_docs(nrtgpu_seg* seg, const uint64_t* bits, int32_t n_words);
/* A new reader version of a sealed segment (what a refresh produces when only liveDocs changed): a handle that SHARES
 * the segment's postings, norms and vectors (nothing is copied or re-uploaded) and carries its own liveDocs (bits as
 * above; NULL = all live) and its own doc-set masks.  Searches over `seg` keep seeing `seg`'s liveDocs -- the
 * point-in-time view an IndexSearcher has in Lucene -- and nobody waits for anybody.  The shared data is freed with the
 * last handle (nrtgpu_segment_release on each).  While a segment has several handles its deletes are tested as a mask
 * instead of being folded into the postings, and -- as in Lucene, where a segment's deletes only accumulate -- a handle's
 * liveDocs may not bring back a doc that the shared postings already carry as deleted (NRTGPU_ERR_UNSUPPORTED). */
int  nrtgpu_segment_fork(nrtgpu_seg* seg, const uint64_t* live_bits, int32_t n_words, nrtgpu_seg** out);
/* Non-scoring clauses as doc-set masks (FILTER / MUST_NOT of the BooleanQuery built at
 * src/main/java/com/yelp/nrtsearch/server/query/QueryNodeMapper.java:257-283).  The shim materialises the
 * clause's per-leaf DocIdSet (what LRUQueryCache caches) as 64-bit words, bit d set = doc d matches,
 * and registers it under an id > 0 of its choosing; queries name ids (nrtgpu_bm25_query.filter_mask /
 * must_not_mask).  bits == NULL drops the mask.  Like set_live_docs: excludes itself from the searches
 * running over this segment.  Bits at or beyond max_doc are ignored. */
int  nrtgpu_segment_set_mask(nrtgpu_seg* seg, int32_t mask_id, const uint64_t* bits, int32_t n_words);
/* A mask BUILT ON THE DEVICE from the segment's resident doc value columns (nrtgpu_segment_add_doc_values / _multi), where the
 * shim would otherwise materialise the clause's DocIdSet on the CPU and upload it: numeric range filters beside a text query
 * ("pizza, rating >= 4"), a kNN pre-filter by a price range, "category in {a, b, c}" over a facet's ordinals (TermInSetQuery /
 * IntPoint.newSetQuery), "has a photo" (FieldExistsQuery).  The mask is the set of docs of this leaf that pass EVERY clause; after
 * the call mask_id behaves exactly as if the caller had computed those words and passed them to nrtgpu_segment_set_mask: usable
 * as filter_mask / must_not_mask / more_* on every route, as a knn pre-filter and a function's filter_mask; replaced by either
 * call and dropped by nrtgpu_segment_set_mask(seg, id, NULL, 0); private to the handle (a fork builds its own, over the shared
 * column).  It does NOT contain liveDocs -- like a cached DocIdSet it is independent of deletes, the routes apply liveDocs
 * themselves.  Bits at or beyond max_doc are 0; *out_count (may be NULL) is the number of set bits.
 * Clauses.  "The column's order" is Integer.compare for ints; for floats the order of
 * NumericUtils.floatToSortableInt(Float.floatToIntBits(.)): -0.0 < +0.0, every NaN the canonical one and above +inf.
 *   NRTGPU_CLAUSE_RANGE   the doc-set range rule, word for word (nrtgpu_range_accepts): the doc has a value with
 *                         lower <= value <= upper, both inclusive; lower > upper matches nothing and is not an error
 *   NRTGPU_CLAUSE_EXISTS  the doc has at least one value; a float NaN is a value
 *   NRTGPU_CLAUSE_IN_SET  the doc has a value whose code equals the code of a listed value [Lucene-recall]: for floats -0.0 and
 *                         +0.0 are different members and any NaN in the list matches every NaN value -- how
 *                         FloatPoint.newSetQuery / IntPoint.newSetQuery compare encoded points (src/main/java/com/yelp/nrtsearch/
 *                         server/field/FloatFieldDef.java:180-182, IntFieldDef.java:174-176).  The values come in any order,
 *                         duplicates allowed
 * Over a MULTI-VALUED column a doc passes a clause iff SOME value of it passes; a doc with no value fails every clause kind.
 * Lifetime and locking are nrtgpu_segment_set_mask's: the call excludes itself from the searches running over this segment and
 * drops the segment's combined accept sets.  It is synchronous: one kernel launch over the columns, the words copied back to the
 * host (where the accept sets are combined, as for every mask); nrtgpu_segment_device_bytes is unchanged by it.  Under
 * nrtgpu_config.collect_timing the kernel's own time is nrtgpu_last_diagnostics' device_ms (total_ms: the call).
 * Refusals, each with a reason in nrtgpu_last_error; all NRTGPU_ERR_INVALID_ARG checks come before any NRTGPU_ERR_UNSUPPORTED
 * one, and a failed call leaves the previous mask under mask_id, if any, untouched:
 *   NRTGPU_ERR_INVALID_ARG  seg or clauses NULL; mask_id <= 0; n_clauses outside 1..NRTGPU_MAX_RANGES; a clause kind outside
 *                           0..2; reserved != 0; IN_SET with n_values outside 1..NRTGPU_MAX_SET_VALUES or value_bits NULL; RANGE
 *                           or EXISTS with n_values != 0 or value_bits non-NULL
 *   NRTGPU_ERR_STATE        the segment is not sealed
 *   NRTGPU_ERR_UNSUPPORTED  a clause's column is not resident on this segment (its kind is then unknown, and a forgotten upload
 *                           must not read as "no doc matches"; a caller who knows the leaf has no value registers zero words
 *                           through nrtgpu_segment_set_mask)
 * 64-bit columns: nrtgpu_segment_set_mask_from_values64 below (this entry refuses them: NRTGPU_ERR_UNSUPPORTED).
 * Out of scope: OR / NOT inside one mask (NOT is must_not_mask at the use site); clauses over postings; zone
 * maps; combining accept sets on the device; the shim's eligibility logic. */
#define NRTGPU_CLAUSE_RANGE  0   /* has a value with lower <= value <= upper (the doc-set range rule, word for word) */
#define NRTGPU_CLAUSE_EXISTS 1   /* has a value (FieldExistsQuery over the doc values) */
#define NRTGPU_CLAUSE_IN_SET 2   /* has a value equal to one of n_values given values (TermInSetQuery) */
#define NRTGPU_MAX_SET_VALUES 4096   /* a design limit: the sorted set is staged in LDS (16 KiB) */
typedef struct {
  int32_t  kind;          /* NRTGPU_CLAUSE_* */
  int32_t  field_id;      /* the column, INT32 or FLOAT32, single- or multi-valued */
  uint32_t lower_bits;    /* RANGE: inclusive, bits of the column's kind; else 0 */
  uint32_t upper_bits;
  int32_t  n_values;      /* IN_SET: 1..NRTGPU_MAX_SET_VALUES; else 0 */
  int32_t  reserved;      /* 0 */
  const uint32_t* value_bits; /* IN_SET: n_values values, bits of the column's kind, any order, duplicates allowed; else NULL */
} nrtgpu_value_clause;    /* 32 bytes */
int  nrtgpu_segment_set_mask_from_values(nrtgpu_seg* seg, int32_t mask_id, const nrtgpu_value_clause* clauses,
                                         int32_t n_clauses /* 1..NRTGPU_MAX_RANGES */, int64_t* out_count /* may be NULL */);
/* The same over 64-BIT columns (nrtgpu_segment_add_doc_values64): "in the last 30 days" over a DATE_TIME column, a price range
 * over a DOUBLE one (LongFieldDef.java:124-154, DateTimeFieldDef.java:133-167: SortedNumericDocValuesField.newSlowRangeQuery).
 * nrtgpu_segment_set_mask_from_values' contract, word for word: the registered mask is usable on every route, independent of
 * liveDocs, bits at or beyond max_doc are 0, a failed call leaves the old mask in place, all NRTGPU_ERR_INVALID_ARG checks come
 * before any NRTGPU_ERR_UNSUPPORTED one, the call is synchronous and reports device_ms under collect_timing.
 *   NRTGPU_CLAUSE_RANGE   the doc has a value with lower <= value <= upper, both inclusive, in the kind's order (Long.compare;
 *                         for doubles the order of NumericUtils.doubleToSortableLong [Lucene-recall]: -0.0 < +0.0, every NaN the
 *                         canonical one and above +inf, so [-inf, +inf] drops the NaN docs and [NaN, NaN] keeps only them);
 *                         lower > upper matches nothing (nrtgpu_range_accepts64)
 *   NRTGPU_CLAUSE_EXISTS  the doc has a value
 * NRTGPU_ERR_INVALID_ARG: seg or clauses NULL; mask_id <= 0; n_clauses outside 1..NRTGPU_MAX_RANGES; a clause kind outside 0..1
 * (no IN_SET); reserved != 0.  NRTGPU_ERR_STATE: the segment is not sealed.  NRTGPU_ERR_UNSUPPORTED: a clause's column is not
 * resident on this segment, or is a 32-bit or multi-valued column (nrtgpu_segment_set_mask_from_values).  "Rating >= 4 AND in
 * the last 30 days" is two masks, named as filter_mask and more_filters. */
typedef struct {
  int32_t  kind;          /* NRTGPU_CLAUSE_RANGE | NRTGPU_CLAUSE_EXISTS */
  int32_t  field_id;      /* the column, INT64 or FLOAT64 */
  uint64_t lower_bits;    /* RANGE: inclusive, bits of the column's kind; else 0 */
  uint64_t upper_bits;
  int64_t  reserved;      /* 0 */
} nrtgpu_value_clause64;  /* 32 bytes */
int  nrtgpu_segment_set_mask_from_values64(nrtgpu_seg* seg, int32_t mask_id, const nrtgpu_value_clause64* clauses,
                                           int32_t n_clauses /* 1..NRTGPU_MAX_RANGES */, int64_t* out_count /* may be NULL */);
/* Whether a 64-bit range clause keeps a doc whose value is value_bits (kind: NRTGPU_DOCVALUES_INT64 / _FLOAT64; *out = 1 / 0),
 * exposed for the tests: needs no device; it is the very function the kernel compiles.  kind outside 2..3 or out NULL:
 * NRTGPU_ERR_INVALID_ARG. */
int  nrtgpu_range_accepts64(int32_t kind, uint64_t lower_bits, uint64_t upper_bits, uint64_t value_bits, int32_t* out);
/* The (max_doc + 63) / 64 words of a registered mask, however it was set (a shim persists a built mask across a fork with it).
 * NRTGPU_ERR_INVALID_ARG: seg or bits NULL, mask_id <= 0, n_words below the need; NRTGPU_ERR_UNSUPPORTED: no mask is registered
 * under the id. */
int  nrtgpu_segment_get_mask(const nrtgpu_seg* seg, int32_t mask_id, uint64_t* bits, int32_t n_words);
void nrtgpu_segment_release(nrtgpu_seg* seg);
/* bytes of HBM held by the segment (diagnostics) */
int64_t nrtgpu_segment_device_bytes(const nrtgpu_seg* seg);

/* ---------------------------------------------------------------------------------------------
 * BM25 disjunction search.  Replaces, for one IndexSearcher.search call: per-leaf
 * Weight.scorerSupplier(ctx).bulkScorer().score(leafCollector, liveDocs, 0, maxDoc) (postings
 * traversal + BM25Similarity SimScorer + double-accumulated disjunction sum), the
 * TopScoreDocCollector / LazyQueueTopScoreDocCollector (src/main/java/org/apache/lucene/search/
 * LazyQueueTopScoreDocCollector.java:103-199) and CollectorManager.reduce == TopDocs.merge
 * (LazyQueueTopScoreDocCollectorManager.java:137-144).
 * Index-global statistics stay on the host: the caller passes weight = boost * idf and the
 * 256-entry normInverse cache of BM25Similarity.scorer() (helpers below compute both).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t field_id;
  int32_t cache_slot;     /* which 256-float table of nrtgpu_bm25_query.norm_cache this term uses */
  int64_t term_hash;
  float   weight;         /* boost * idf, float (BM25Similarity.scorer) */
  int32_t occur;          /* 0: SHOULD; 1: MUST (BooleanClause.Occur, QueryNodeMapper.java:257-283).  Every clause MUST: the
                           * conjunction (all clauses match, score = (float) of the double sum -- ConjunctionScorer), the same as
                           * min_should_match = n_terms over SHOULD clauses.  MUST next to SHOULD clauses (min_should_match 0):
                           * a hit matches every MUST clause and scores (float) sum of the MUST scores + (float) sum of its
                           * matching SHOULD scores, the two added in float (ReqOptSumScorer [Lucene-recall]); MaxScore route
                           * only (<= 8 clauses, fixed-point sums, not ScoreMode.COMPLETE on a large query), else
                           * NRTGPU_ERR_UNSUPPORTED; with min_should_match > 0 or disjunction_max: NRTGPU_ERR_UNSUPPORTED */
} nrtgpu_term;

typedef struct {
  int32_t n_terms;                 /* 1..NRTGPU_MAX_TERMS SHOULD clauses (duplicates allowed) */
  const nrtgpu_term* terms;
  int32_t n_caches;                /* number of 256-float tables in norm_cache (one per field) */
  const float* norm_cache;         /* n_caches * 256 floats */
  int32_t k;                       /* numHits, 1..NRTGPU_MAX_K  (DocCollector.java:79-114) */
  int32_t total_hits_threshold;    /* >= 0; INT32_MAX => exact count (ScoreMode.COMPLETE) */
  int32_t has_after;               /* searchAfter (LazyQueueTopScoreDocCollector.java:112-120) */
  int32_t after_doc;               /* global docid of the last hit of the previous page */
  float   after_score;
  int32_t min_should_match;        /* minimumNumberShouldMatch (QueryNodeMapper.java:259-261): 0 and 1 are the plain
                                    * disjunction; > 1: only docs matched by that many clauses are hits, the score
                                    * is still the sum over all matching clauses (what Lucene's WANDScorer returns).
                                    * > 1 on the exhaustive route needs the fixed-point accumulators for the whole batch,
                                    * else NRTGPU_ERR_UNSUPPORTED (nrtgpu_search_bm25_coalesced: for that request only) */
  float   min_competitive_score;   /* Scorable.setMinCompetitiveScore across shards: a lower bound of the k-th best
                                    * score of the WHOLE search this call is one shard of (other GPUs' results so
                                    * far, LazyMaxScoreAccumulator).  Docs scoring strictly below it are counted in
                                    * total_hits but not collected; 0 = none */
  int32_t filter_mask;             /* 0 = none; else hits must lie in this registered mask on every segment: a
                                    * FILTER clause next to the SHOULD clauses with minimumNumberShouldMatch = 1,
                                    * or "+(should clauses) #filter" -- either way a hit matches >= 1 scoring
                                    * clause and the filter adds nothing to the score */
  int32_t must_not_mask;           /* 0 = none; else hits must NOT lie in this mask (MUST_NOT clause) */
  int32_t disjunction_max;         /* 0: BooleanQuery, a doc scores the sum of its matching clauses.
                                    * 1: DisjunctionMaxQuery over the same term clauses (src/main/java/com/yelp/nrtsearch/
                                    * server/query/QueryNodeMapper.java:350-358): a doc scores its BEST matching clause plus
                                    * tie_breaker x the others.  Fixed-point sums (on the exhaustive route: for the whole batch), else
                                    * NRTGPU_ERR_UNSUPPORTED; min_should_match <= 1, every clause SHOULD; disjuncts that are
                                    * not term queries stay on the caller's path */
  int32_t n_more_filters;          /* further FILTER clauses next to filter_mask (QueryNodeMapper.java:257-283 builds any number): */
  const int32_t* more_filters;     /* ... resident mask ids > 0; a hit lies in ALL of the query's filter masks */
  int32_t n_more_must_not;         /* further MUST_NOT clauses next to must_not_mask: */
  const int32_t* more_must_not;    /* ... resident mask ids > 0; a hit lies in NONE of the query's must_not masks.  The masks are
                                    * combined at plan time (one AND / AND NOT pass over 64-bit words per leaf and combination,
                                    * cached on the segment like a single pair); n_more_* = 0: the arrays are not read */
  float   tie_breaker;             /* DisjunctionMaxQuery.tieBreakerMultiplier, 0..1 (disjunction_max = 1 only, else 0): the score
                                    * is (float)(scoreMax + otherScoreSum * tieBreaker) in double, as DisjunctionMaxScorer
                                    * computes it [Lucene-recall]; 0 is what the reference's own test uses (src/test/java/com/
                                    * yelp/nrtsearch/server/grpc/QueryTest.java:541-583).  > 0: MaxScore route only (see
                                    * nrtgpu_term.occur), else NRTGPU_ERR_UNSUPPORTED */
  int32_t reserved;
} nrtgpu_bm25_query;

typedef struct {
  int32_t  n_hits;                     /* out: hits written, <= k */
  int32_t  capacity;                   /* in : capacity of docs/scores (>= k) */
  int32_t* docs;                       /* out: global docids (doc_base + leaf doc) */
  float*   scores;                     /* out: (score desc, doc asc) */
  int64_t  total_hits;                 /* out: live matching docs: the exact number, or -- when the query ran with dynamic pruning
                                        * (MaxScore route; total_hits_is_lower_bound = 1) -- a lower bound above totalHitsThreshold.
                                        * WHICH lower bound: where the planner knew beforehand that some slice passes the threshold
                                        * (a plain disjunction whose largest term alone does), the live docs it knew to match -- the
                                        * same number on every run; where the query had to count its way to the threshold (masks,
                                        * minimumNumberShouldMatch, DisjunctionMax, an uncertain count), the docs the walk had
                                        * evaluated -- which depends on when its workgroups saw the threshold passed and on what the
                                        * bounds then skipped: NOT the same from run to run (Lucene's own value there is an artefact
                                        * of its traversal too).  The relation and the returned hits are deterministic either way. */
  int32_t  total_hits_is_lower_bound;  /* out: 1 == GREATER_THAN_OR_EQUAL_TO: some slice of the searcher (nrtgpu_set_slicing)
                                        * collected more than max(totalHitsThreshold, numHits) hits and numHits hits were returned */
} nrtgpu_topdocs;

/* Slicing of the searcher this context serves (MyIndexSearcher.SlicingParams: the index live settings sliceMaxDocs,
 * sliceMaxSegments, virtualShards; src/main/java/com/yelp/nrtsearch/server/search/MyIndexSearcher.java:79-208).  The
 * reference runs one collector per slice and merges: TotalHits.relation is GREATER_THAN_OR_EQUAL_TO iff SOME SLICE
 * collected more than max(totalHitsThreshold, numHits) hits (LazyQueueTopScoreDocCollector.java:176-199 per slice,
 * LazyQueueTopScoreDocCollectorManager.java:137-144) -- 1500 hits spread over ten slices are EQUAL_TO 1500.  The
 * library derives the same slices from the leaves of each call (maxDoc, live docs, docBase) and reports the relation
 * by that rule; dynamic pruning is used only where some slice certainly passes the threshold.  Defaults: 250000, 5, 1.
 * slice_max_docs == 0: the whole search counts as one slice. */
int  nrtgpu_set_slicing(nrtgpu_ctx* ctx, int32_t slice_max_docs, int32_t slice_max_segments, int32_t virtual_shards);
/* PARTIAL RESIDENCY ("non-resident segments are searched by Lucene and merged with TopDocs.merge").  Under NRT refresh a
 * searcher usually holds a few young segments that are not resident yet (ShardState.java:506-527).  The caller then splits the
 * searcher's SLICES (IndexSearcher.getSlices(), MyIndexSearcher.java:79-208): the slices whose leaves are all resident go to
 * nrtgpu_search_bm25* in ONE call over their leaves, the other slices run through Lucene's own collectors, and the per-slice
 * results are reduced as the reference reduces them -- TopDocs.merge, totalHits summed, GREATER_THAN_OR_EQUAL_TO if any part's is
 * (LazyQueueTopScoreDocCollectorManager.java:137-144).  Statistics stay index-global (the weights the caller passes).
 * A call over a SUBSET of the searcher's leaves must count its hits by the WHOLE searcher's slices: with the default slicing the
 * library's own slicing of whole slices' leaves reproduces them (leaves are packed in size order; a removed slice removes a whole
 * run), with virtual shards it does not (leaves are dealt to shards over all leaves first).  So the calling thread may state the
 * slice of every leaf of its next calls: slice_of_leaf[i] >= 0 for the call's i-th leaf (any numbering; equal numbers = one slice),
 * n_leaves = the call's leaf count (a call with another count ignores the override and slices by itself); NULL / 0 clears it.
 * Thread-local, like the deadline: set before the search call, cleared after. */
int  nrtgpu_set_thread_slices(const int32_t* slice_of_leaf, int32_t n_leaves);

int  nrtgpu_search_bm25(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                        const nrtgpu_bm25_query* q, nrtgpu_topdocs* out);
/* The eligibility test alone (the predicate a GpuIndexSearcher applies to the rewritten query before it
 * chooses between this library and super.search): NRTGPU_OK if nrtgpu_search_bm25 would run `q` over these leaves,
 * else the status it would return (NRTGPU_ERR_UNSUPPORTED: too many clauses / fields, numHits > NRTGPU_MAX_K, a mask
 * that is not resident on a leaf, minimumNumberShouldMatch > 1 without the fixed-point range, ...) with the reason
 * in nrtgpu_last_error().  No device work. */
int  nrtgpu_query_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q);
/* n_queries independent searches over the same leaves in one device pass */
int  nrtgpu_search_bm25_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                              const nrtgpu_bm25_query* queries, int32_t n_queries, nrtgpu_topdocs* out);

/* The same single search, but concurrent callers (the SEARCH / gRPC pool's threads, each blocked in its own
 * call: SearchHandler.java:1412 runs on the request thread) are coalesced by the library into device batches:
 * a caller that finds no batch forming waits at most `linger_us` (default 150) for company -- less when, with nothing in
 * flight, as many callers wait as the last batch held (the cohort of a closed loop is back) -- then runs everybody's
 * queries over the same leaves as one batch.  No extra thread; results identical to nrtgpu_search_bm25. */
int  nrtgpu_search_bm25_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                  const nrtgpu_bm25_query* q, nrtgpu_topdocs* out);
int  nrtgpu_set_coalescing(nrtgpu_ctx* ctx, int32_t linger_us);
/* Speculative thresholds of the MaxScore route (nrtgpu_search_bm25 / _batch / _coalesced / nrtgpu_search_hybrid_batch
 * -- the calls that can run a query again): a workgroup that has walked a fraction of a query's docs guesses the final k-th score from the best of what
 * it has seen, `margin` standard deviations on the safe side, and skips what cannot reach the guess; the merge checks every
 * guess against the merged list and a query whose guess failed is run again without speculation inside the same call.  Results
 * are exact either way.  margin 0 switches it off; a context starts with 5.  The library judges every leaf set (the segments of
 * one searcher version) by its own failures: more than 2 % of >= 2048 queries run again moves the leaf set to a scattered window
 * order, and if the guesses fail there too speculation is switched off for it.  Resets the counters nrtgpu_get_stats reports
 * (spec_queries / spec_reruns / spec_scattered / spec_disabled) and every leaf set's verdict. */
int  nrtgpu_set_speculation(nrtgpu_ctx* ctx, float margin);

/* Device-resident variant for the multi-GPU path (one process per GPU): results stay
 * in HBM as packed keys so the caller can RCCL all-gather them without a host round trip.
 *   d_keys  : n_queries * k_stride uint64 (device), key = (float_bits(score) << 32) | (0xFFFFFFFF - doc),
 *             sorted descending == (score desc, doc asc); unused tail slots are 0
 *   d_counts: n_queries uint32 (device) hits per query
 *   d_hits  : n_queries uint64 (device) total hits per query: the exact count, or -- for a query that ran with dynamic
 *             pruning -- (1 << 48) + a lower bound above totalHitsThreshold; sums of these over shards keep both
 *             parts, and nrtgpu_merge_topk_device reports such a sum as GREATER_THAN_OR_EQUAL_TO
 * Returns after the work is enqueued AND complete on the library's stream (synchronous). */
int  nrtgpu_search_bm25_batch_device(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                                     int32_t n_segs, const nrtgpu_bm25_query* queries, int32_t n_queries,
                                     int32_t k_stride, void* d_keys, void* d_counts, void* d_hits);
/* The same in two halves, for callers that pipeline: _begin plans the batch, enqueues its kernels on one of the library's streams
 * and returns at once (the plan, the workspace and shared locks on the segments' content stay with the pending handle);
 * nrtgpu_pending_wait blocks until the results are complete in d_keys / d_counts / d_hits and releases everything.  ONE
 * submitting thread then keeps the device fed -- the plan of batch i + 1 is built while the kernels of batch i run -- and
 * nobody spins on a stream in between (a rank of a multi-GPU job: ~1 CPU instead of one per call in flight).  At most 4
 * batches in flight per context (a fifth _begin waits for a workspace); every handle must be waited for exactly once.
 * epoch: as nrtgpu_search_bm25_batch_device_epoch below (-1: no bound exchange). */
/* Lifetime contract of a pending search: it holds its segments' content from begin to wait (set_live_docs / set_mask on those
 * handles wait for it; nrtgpu_segment_release is deferred to it).  nrtgpu_pending_wait may be called from any thread.  A thread
 * that holds un-waited pending searches may begin more (they pass a writer that is waiting for the earlier ones) but must not
 * start a SYNCHRONOUS search over the same handles before it has waited: that one queues behind the waiting writer. */
typedef struct nrtgpu_pending nrtgpu_pending;
int  nrtgpu_search_bm25_batch_device_begin(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                                           int32_t n_segs, const nrtgpu_bm25_query* queries, int32_t n_queries,
                                           int32_t k_stride, void* d_keys, void* d_counts, void* d_hits, int64_t epoch,
                                           nrtgpu_pending** out);
int  nrtgpu_pending_wait(nrtgpu_pending* pending);
/* One SHARD of a search that `spec_world` GPUs share by equal docid ranges (the multi-GPU form below, for callers that pipeline
 * it themselves): as nrtgpu_search_bm25_batch_device_begin without an epoch, but the speculative thresholds of this call are
 * guesses at the k-th score of the WHOLE search -- a shard's docs are a 1 / spec_world sample of the index, so after a fraction f
 * of its windows it holds about k f / spec_world of the final top-k and the (that + z sd + 2)-th best key it has seen is the
 * guess (csrc/maxscore.hip: ms_compact).  Every shard then collects about k / spec_world candidates instead of k and no bound
 * travels between the GPUs while they walk.  A guess can only be checked against the MERGED list: the largest guess per query is
 * left in d_guess (n_queries x u64 in HBM, 0: none) -- nrtgpu_dist_exchange_merge_checked takes it along, checks it and says
 * which queries every shard has to run again (spec_world 0: without speculation).  The results are exact either way.
 * spec_world counts shards OF THIS SHARD'S SIZE: total docs / this shard's docs, rounded down.  A shard that holds more of the
 * index than it says guesses too high -- its guesses are caught by the check and cost re-runs, never a wrong answer
 * (nrtgpu_dist_search_bm25_batch_mode passes the communicator's size: docid-range shards are equal to within a segment boundary).
 * nrtgpu_note_shard_speculation tells the leaf set's verdict (nrtgpu_stats.spec_*) how a batch went, for callers that do the
 * check themselves; nrtgpu_dist_search_bm25_batch_mode does all of this itself. */
/* The share of a sharded index this context holds (round 6): shard_docs of index_docs live docs.  Where it is set, the guesses of
 * the shard-level speculation (nrtgpu_search_bm25_shard_device_begin with spec_world >= 2, nrtgpu_dist_search_bm25_batch[_mode])
 * count "the windows of all shards" as this shard's windows x index_docs / shard_docs instead of x spec_world: the reference's
 * virtual shards balance LIVE docs by greedy LPT over whole segments (MyIndexSearcher.java:117-160), which leaves shards of 40 %
 * and 20 % of an index side by side, and a shard that holds more than 1 / spec_world of the docs guesses too high (caught by the
 * check, but every catch is a second pass).  (0, 0): equal shards again.  Changes nothing but how often guesses fail. */
int  nrtgpu_set_shard_share(nrtgpu_ctx* ctx, int64_t shard_docs, int64_t index_docs);
int  nrtgpu_search_bm25_shard_device_begin(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                           const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t k_stride, void* d_keys,
                                           void* d_counts, void* d_hits, int32_t spec_world, void* d_guess, nrtgpu_pending** out);
int  nrtgpu_note_shard_speculation(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, int32_t n_queries, int32_t n_failed);
/* Cross-GPU bound exchange (the LazyMaxScoreAccumulator idea across processes, SURVEY 8e "optional cross-GPU
 * theta sharing").  When one search is sharded over `world` GPUs, every shard alone would converge on the
 * k-th best of ITS docs.  With an exchange open, each shard publishes a score that at least
 * ceil(k / (world - 1)) of its docs reach; the entries of any world - 1 shards then cover k docs, so a shard
 * needs to collect nothing below the smallest entry of the OTHER shards.  Results of the merged search are unchanged
 * (tests/test_exchange_gpu.py); shards return fewer low-ranked hits.
 * The table lives in POSIX shared memory `shm_name` (every rank passes the same name; rank 0 should
 * unlink stale files first), mapped into each process's GPU.  Ranks must synchronise once between
 * nrtgpu_exchange_open and their first search.  Batches are matched across ranks by `epoch` (same
 * queries in the same order on every rank, epochs increasing; ranks may run up to 6 epochs apart). */
int  nrtgpu_exchange_open(nrtgpu_ctx* ctx, const char* shm_name, int32_t world, int32_t rank);
void nrtgpu_exchange_close(nrtgpu_ctx* ctx);
int  nrtgpu_search_bm25_batch_device_epoch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                                           int32_t n_segs, const nrtgpu_bm25_query* queries, int32_t n_queries,
                                           int32_t k_stride, void* d_keys, void* d_counts, void* d_hits, int64_t epoch);

/* The multi-GPU search with the collective INSIDE the library (a JVM caller has no torch): one process per GPU, every
 * rank holds a docid-range shard of the index.  nrtgpu_dist_unique_id on one rank (128 bytes: an ncclUniqueId), the bytes
 * travel to the other ranks by whatever means the deployment has, nrtgpu_dist_init on every rank (ncclCommInitRank on the
 * context's device; RCCL is bound at run time with dlopen, NRTGPU_ERR_UNSUPPORTED if it is not installed).  Then every
 * rank calls nrtgpu_dist_search_bm25_batch with the same queries in the same order (index-global statistics in the
 * weights) over ITS leaves: local search -> ONE grouped RCCL all-gather of keys / counts / hit totals over xGMI ->
 * TopDocs.merge on every rank; every rank receives every answer.  total_hits sums the shards' counts; the relation is
 * GREATER_THAN_OR_EQUAL_TO iff some shard's is.
 * Failure of ONE rank's part of a one-call search (nrtgpu_dist_search_bm25_batch[_mode], nrtgpu_dist_knn_exact,
 * nrtgpu_dist_search_hybrid_batch) -- its thread's deadline, a planner refusal, a device error: every rank issues the same
 * collectives whatever fails; a failed rank skips its remaining local steps and enters each exchange with empty lists and its
 * status word in the same collective.
 *   - a failure BEFORE the call's last exchange (the local search, BM25's merge and verdicts when the all-to-all form's verdict
 *     all-gather follows, BM25's re-run, the hybrid's first-pass merge and tail): EVERY rank returns an error (the failed rank its
 *     own, the others NRTGPU_ERR_STATE naming the first failed rank), and the communicator stays usable;
 *   - a failure AFTER it (the final merge): that rank's alone -- it returns its error, its peers return their answers;
 *   - in either case no rank waits in a collective a peer will not issue.  Two cases are left out by design: a failure to
 *     reserve the call's buffers (before any collective: that rank leaves before the first exchange -- after the first call of
 *     a shape this cannot happen), and, when the lists are gathered whole (the all-gather form, or a batch the all-to-all form
 *     cannot slice: nrtgpu_dist_owned_range), a failure of BM25's merge on one rank after an exchange in which every rank
 *     succeeded, while queries are to be run again: that rank cannot know whether its peers will re-run, and closing this
 *     would take one more collective on every speculating call.
 * The re-run of queries whose speculative threshold failed ignores the thread's deadline (it is the tail of a search that was
 * launched in time).  A caller that pipelines with the two halves below vouches for its own ranks: nothing of this travels there. */
int  nrtgpu_dist_unique_id(void* out128);
int  nrtgpu_dist_init(nrtgpu_ctx* ctx, int32_t world, int32_t rank, const void* id128);
int  nrtgpu_dist_search_bm25_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                   const nrtgpu_bm25_query* queries, int32_t n_queries, nrtgpu_topdocs* out);
/* The exchange stage on its own, for callers that pipeline (host threads run nrtgpu_search_bm25_batch_device[_epoch] ahead,
 * one thread issues the exchanges in batch order -- the same order on every rank): this rank's device-resident shard
 * results (keys n_queries x k_stride, counts, hit totals) -> grouped all-gather -> TopDocs.merge into `out`. */
int  nrtgpu_dist_allgather_merge(nrtgpu_ctx* ctx, int32_t n_queries, int32_t k_stride, const void* d_keys, const void* d_counts,
                                 const void* d_hits, const int32_t* ks, const int32_t* total_hits_thresholds, nrtgpu_topdocs* out);
/* Who receives which answer.  ALLGATHER (BASELINE.json's north star, and what the two calls above do): every rank merges every
 * query and holds every answer.  ALLTOALL: rank r receives every rank's lists for ITS slice of the batch -- queries
 * [r * n / world, (r + 1) * n / world) -- and merges only those: 1 / world of the bytes on every xGMI link (point-to-point
 * links: what an all-to-all wants), of the merge and of the host-side unpacking; the rank that owns a query answers its caller.
 * `out` always has n_queries entries, indexed like the batch; entries of queries this rank does not own come back with
 * n_hits = 0, total_hits = -1.  A batch the ranks cannot share evenly (n_queries % world != 0), or an RCCL without
 * ncclSend / ncclRecv, is gathered whole: nrtgpu_dist_owned_range says what a call will deliver. */
#define NRTGPU_EXCHANGE_ALLGATHER 0
#define NRTGPU_EXCHANGE_ALLTOALL 1
#define NRTGPU_EXCHANGE_NO_SPECULATION 0x100   /* or-ed into nrtgpu_dist_search_bm25_batch_mode's mode: no shard-level guesses */
int  nrtgpu_dist_owned_range(nrtgpu_ctx* ctx, int32_t n_queries, int32_t mode, int32_t* first_query, int32_t* n_owned);
int  nrtgpu_dist_search_bm25_batch_mode(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                        const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t mode, nrtgpu_topdocs* out);
int  nrtgpu_dist_exchange_merge(nrtgpu_ctx* ctx, int32_t n_queries, int32_t k_stride, const void* d_keys, const void* d_counts,
                                const void* d_hits, const int32_t* ks, const int32_t* total_hits_thresholds, int32_t mode,
                                nrtgpu_topdocs* out);
/* The same with the shards' speculative thresholds (d_guess of nrtgpu_search_bm25_shard_device_begin; NULL: the call above): the
 * guesses travel in the same grouped collective as the lists, and after the merge the k-th key of every merged list is checked
 * against the largest guess any shard published for the query (the k-th key is read from the MERGED keys, never from `out`'s
 * arrays: those may be NULL or shorter than k).  failed[n_queries] / *n_failed: the queries whose answer does
 * NOT stand -- the same verdicts on every rank (all-to-all: the owners' verdicts are all-gathered, one byte per query) -- to be
 * run again by EVERY rank without speculation (nrtgpu_dist_search_bm25_batch_mode with NRTGPU_EXCHANGE_NO_SPECULATION over
 * those queries, in the same order on every rank). */
int  nrtgpu_dist_exchange_merge_checked(nrtgpu_ctx* ctx, int32_t n_queries, int32_t k_stride, const void* d_keys, const void* d_counts,
                                        const void* d_hits, const void* d_guess, const int32_t* ks, const int32_t* total_hits_thresholds,
                                        int32_t mode, nrtgpu_topdocs* out, uint8_t* failed, int32_t* n_failed);
/* Exact vector search over a row-partitioned field (BASELINE config 4: 10M x 768 over 1..8 GPUs): every rank scores the rows of
 * ITS leaves (nrtgpu_knn_exact on its shard, results kept in HBM), the per-rank top-k lists are exchanged and merged like the
 * BM25 ones -- NrtKnnFloatVectorQuery's per-leaf merge (src/main/java/com/yelp/nrtsearch/server/query/vector/
 * NrtKnnFloatVectorQuery.java:60-64; request glue: search/KnnUtils.java:47-66) taken across GPUs.  Every rank passes the same
 * queries; total_hits = the live vectors of all shards. */
int  nrtgpu_dist_knn_exact(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                           int32_t sim, const float* queries, int32_t n_queries, int32_t dim, int32_t k, float boost, int32_t mode,
                           nrtgpu_topdocs* out /* n_queries */);
/* The hybrid (BASELINE config 5: BM25 recall + vector rescore over 1..8 GPUs) on docid-range shards.  Every rank passes the same
 * queries and query vectors and ITS leaves: BM25 recall on every shard -> ONE all-gather + merge on every rank (the GLOBAL first
 * pass: a doc of a shard's list that did not make the merged list must not be rescored) -> every rank rescores ITS docs of the
 * merged lists against its resident vectors -> the rescored windows are exchanged (`mode`) and merged.  Same answers as
 * nrtgpu_search_hybrid_batch over the whole index; total_hits / relation are the first pass's. */
int  nrtgpu_dist_search_hybrid_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                     const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t field_id, int32_t sim,
                                     const float* query_vectors, int32_t dim, float boost, double query_weight, double rescore_weight,
                                     int32_t window, int32_t mode, nrtgpu_topdocs* out /* n_queries, capacity >= window */);
void nrtgpu_dist_close(nrtgpu_ctx* ctx);

/* TopDocs.merge of n_lists per-GPU results laid out as the all-gather leaves them:
 * d_keys_in[list][query][k_stride], d_counts_in[list][query], d_hits_in[list][query] (device).
 * Writes host-side topdocs (docs/scores/total_hits/relation) for each query.  total_hits = the sum of the lists' counts;
 * the relation is GREATER_THAN_OR_EQUAL_TO iff some list's count carries the tag (a slice of that shard passed the
 * threshold, or the shard pruned) and numHits hits are returned.  total_hits_thresholds is kept for the signature. */
int  nrtgpu_merge_topk_device(nrtgpu_ctx* ctx, int32_t n_lists, int32_t n_queries, int32_t k_stride,
                              const void* d_keys_in, const void* d_counts_in, const void* d_hits_in,
                              const int32_t* ks, const int32_t* total_hits_thresholds, nrtgpu_topdocs* out);

/* ---------------------------------------------------------------------------------------------
 * Exact (brute-force) float vector search.  Replaces ExactFloatVectorQuery's scorer loop
 * (src/main/java/com/yelp/nrtsearch/server/query/vector/ExactVectorQuery.java:137-173: score =
 * VectorSimilarityFunction.compare(query, docVector) * boost for every doc that has a vector) plus
 * the top-k collector behind it; also the exact reading of the `knn` request path (recall 1.0;
 * compare against ExactFloatVectorQuery, not HNSW).
 *   sim: 0 cosine, 1 dot_product (unit vectors; also "normalized_cosine"), 2 l2_norm, 3 max_inner_product
 *        (mapping: src/main/java/com/yelp/nrtsearch/server/field/VectorFieldDef.java:77-88)
 *   queries: n_queries * dim fp32, row-major (already normalised by the caller where the field asks
 *        for it, VectorFieldDef.java:564-573)
 * Scores are fp32 sums in MFMA order: equal to Lucene within 1e-5 relative (Lucene's own order
 * depends on the JVM's vector width); docids ranked by (score desc, doc asc).  l2_norm: the squared distance is taken
 * as |q|^2 + |v|^2 - 2 q.v (one pass over the rows for every query of the batch), whose rounding error is
 * ~1e-7 * (|q|^2 + |v|^2): for near-duplicate vectors of large norm that exceeds 1e-5 of a tiny distance -- the
 * tolerance claim holds for the score 1 / (1 + d^2) (absolute 1e-4, tests/test_vectors_gpu.py), not for d^2 itself.
 * --------------------------------------------------------------------------------------------- */
int  nrtgpu_knn_exact(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                      int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim, int32_t k,
                      float boost, nrtgpu_topdocs* out /* n_queries */);

/* What a request thread calls with ONE exact vector query (ExactFloatVectorQuery, query/vector/ExactVectorQuery.java:179-196):
 * blocks; concurrent callers over the same leaves, field, similarity and boost are merged into panels of up to 64 queries that
 * share one pass over the rows (a pass costs the same for 1 query as for 64).  Leader / follower, no extra thread: a caller that
 * finds the device free runs at once with whatever is waiting (a lone caller pays no batching latency); while a panel runs,
 * arrivals accumulate and leave together when it finishes, or as a second panel in flight once 64 are waiting.  A panel is
 * searched with the largest k of its members; each gets the first k of its own.  Results, errors and deadlines
 * (NRTGPU_ERR_TIMEOUT for a request that expired while waiting) as nrtgpu_knn_exact with n_queries = 1. */
int  nrtgpu_knn_exact_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                int32_t field_id, int32_t similarity, const float* query, int32_t dim, int32_t k, float boost,
                                nrtgpu_topdocs* out);
/* TotalHits.relation of an exact vector query as the reference reports it.  The count is exact either way (the scorer ignores
 * min competitive scores: every live doc with a vector is collected), but the reference's collector still flips its relation to
 * GREATER_THAN_OR_EQUAL_TO once a slice has collected more than max(totalHitsThreshold, numHits) hits with a full queue
 * (LazyQueueTopScoreDocCollector.java:176-199, one collector per slice: MyIndexSearcher.java:163-208).  Host only: the live
 * vectors of every leaf are known from upload and liveDocs.  Returns 1 = GREATER_THAN_OR_EQUAL_TO, 0 = EQUAL_TO, < 0 = error. */
int  nrtgpu_knn_exact_relation(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                               int32_t field_id, int32_t k, int32_t total_hits_threshold);
/* The `knn` request path (KnnQuery -> NrtKnnFloatVectorQuery, src/main/java/com/yelp/nrtsearch/server/field/
 * VectorFieldDef.java:564-594, executed at search/KnnUtils.java:56) answered exactly: the k nearest docs among
 * those the pre-filter accepts (filter_mask: a resident mask, 0 = none; liveDocs always apply), optionally only
 * docs whose unboosted score is >= min_score (the MinThresholdQuery wrapped around the knn query at
 * VectorFieldDef.java:591-594; the caller converts similarityThreshold with similarityToScore, :664-673;
 * 0 = none), scores multiplied by boost afterwards.  total_hits = hits returned, as for the rewritten
 * knn query.  Recall is 1.0 where the reference's HNSW walk is approximate. */
int  nrtgpu_knn_search(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                       int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim, int32_t k,
                       float boost, int32_t filter_mask, float min_score, nrtgpu_topdocs* out /* n_queries */);

/* ---------------------------------------------------------------------------------------------
 * knn requests that share a pass although each has a pre-filter, threshold, k and boost of its OWN (float fields).
 * nrtsearch sends one `knn` request per search thread, each with its own filter (VectorFieldDef.java:580-594, run at
 * search/KnnUtils.java:56): through nrtgpu_knn_search every one of them pays a pass over the rows alone, and a pass costs the
 * same for 1 query as for 64.  The two entries below answer up to 64 such requests per pass.
 * n_queries `knn` requests over the same leaves, field and similarity, each with its OWN k, pre-filter, threshold and boost,
 * answered in passes of up to 64 queries that share one read of the rows.  Query i gets exactly what
 * nrtgpu_knn_search(..., queries + i*dim, 1, dim, ks[i], boosts[i], filter_masks[i], min_scores[i], &out[i]) returns:
 * same docids, ranks, score bits, total_hits (= the hits returned; liveDocs always apply).
 * A pass is searched with the largest k of its members and scores unboosted; member i takes the first ks[i] hits of its list
 * and its own boost when the list is unpacked.  On the device a pass brings a table of accept sets (liveDocs & the member's
 * filter, per leaf and member) and the members' thresholds; a call whose requests are all equal is nrtgpu_knn_search itself,
 * the gather route (nrtgpu_set_knn_gather) included.
 * Refusals, per request, are nrtgpu_knn_search's.  NRTGPU_ERR_INVALID_ARG: k <= 0, filter_mask < 0, a min_score that is not
 * >= 0, a boost that is not finite and > 0, a query dimension other than the field's, a byte field (these are float entry
 * points), ks == NULL.  NRTGPU_ERR_UNSUPPORTED: k > NRTGPU_MAX_K, dim > 2048, a mask that is not resident on a leaf of the call
 * that holds the field's rows.  NULL boosts: all 1; NULL filter_masks: none; NULL min_scores: none.  A bad request refuses the
 * WHOLE call of the batch entry before anything is launched, and nrtgpu_last_error names it ("query <i>: ...").
 * Thread deadlines: checked on entry and between passes.
 * nrtgpu_get_stats: a pass counts under knn_panels / knn_rows / knn_score_launches / knn_score_ms / knn_sketch_launches /
 * knn_second_passes like a pass of nrtgpu_knn_search.
 * Byte fields: the twins nrtgpu_knn_search_bytes_requests / nrtgpu_knn_search_bytes_coalesced further down (these two refuse a
 * byte field by name).
 * Out of scope: the nrtgpu_dist_* forms, the gather route for a pass whose members name different filters (it always passes
 * over all rows), MUST_NOT masks or several filters per request, and the Java shim.
 * --------------------------------------------------------------------------------------------- */
int  nrtgpu_knn_search_requests(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim,
                                const int32_t* ks, const float* boosts, const int32_t* filter_masks, const float* min_scores,
                                nrtgpu_topdocs* out /* n_queries; out[i].capacity >= ks[i] */);
/* What a request thread calls with ONE knn request: blocks; concurrent callers over the same leaves, doc_bases, field,
 * similarity and dimension share panels of up to 64 whatever their k, filter, threshold and boost.  The leave rule and the caps
 * are nrtgpu_knn_exact_coalesced's (a queue of its own: the two entries' callers never share a panel).  A bad request -- the
 * refusals above, its mask's residency on every leaf included -- fails ALONE, before it is queued; a request whose thread
 * deadline passes in the queue returns NRTGPU_ERR_TIMEOUT ("deadline passed while the request waited for a panel"). */
int  nrtgpu_knn_search_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                 int32_t field_id, int32_t sim, const float* query, int32_t dim, int32_t k, float boost,
                                 int32_t filter_mask, float min_score, nrtgpu_topdocs* out);

/* ---------------------------------------------------------------------------------------------
 * Exact search over BYTE (int8) vector fields (nrtgpu_segment_add_byte_vectors).
 * nrtgpu_knn_exact_bytes replaces ExactVectorQuery.ExactByteVectorQuery (query/vector/ExactVectorQuery.java:230-247) as
 * nrtgpu_knn_exact replaces the float query; nrtgpu_knn_search_bytes answers the `knn` request path over a byte field
 * (NrtKnnByteVectorQuery, VectorFieldDef.java:789-829) exactly, as nrtgpu_knn_search does: pre-filter mask, min_score on the
 * UNBOOSTED score, boost afterwards, total_hits = hits returned.  queries: n_queries * dim int8, row-major.
 *   sim: 0 cosine, 1 dot_product, 2 l2_norm, 3 max_inner_product ("normalized_cosine" does not exist for byte fields:
 *        VectorFieldDef.java:698-701)
 * The unboosted score of a (query, row) pair, from the INTEGERS dot = sum q_i v_i, nq = sum q_i^2, nv = sum v_i^2 (int32; below
 * 2^28 at dim <= 2048) -- all float32, each operation rounded once, int -> float conversions round to nearest even.  The four
 * shapes are ByteVectorFieldDef.similarityToScore (VectorFieldDef.java:870-881); how Lucene's
 * VectorSimilarityFunction.compare(byte[], byte[]) reaches them is [Lucene-recall] like the rest of the vector arithmetic
 * (SURVEY A.7):
 *   cosine            c = (float)((double)dot / sqrt((double)nq * (double)nv));  (1.0f + c) / 2.0f
 *   dot_product       0.5f + (float)dot / (float)(dim * 32768)      (dim: the field's own dimension)
 *   l2_norm           d2 = nq + nv - 2 * dot (int32, == sum (q_i - v_i)^2);  1.0f / (1.0f + (float)d2)
 *   max_inner_product x = (float)dot;  x < 0 ? 1.0f / (1.0f + -1.0f * x) : x + 1.0f
 * Returned score = unboosted score * boost (float), as VectorValuesScorer.score() (ExactVectorQuery.java:165-167).  The matrix
 * cores return the integers exactly, so these are final score bits from ONE pass over the rows: no tolerance, no second pass.
 * Cosine: a zero QUERY is refused (NRTGPU_ERR_INVALID_ARG; validateVectorForSearch, VectorFieldDef.java:853-861).  A zero ROW
 * cannot exist in a cosine field of the reference (the same check at indexing, :750), but the library does not know a field's
 * similarity at upload: such a row scores 0 under sim = 0 (never NaN, never a fault).
 * boost: finite and >= 0 (else NRTGPU_ERR_INVALID_ARG: hits are ranked through keys that order like non-negative scores).
 * Otherwise the float entries' contract: ranking (score desc, doc asc), global docids, liveDocs always apply, k <= NRTGPU_MAX_K
 * (else NRTGPU_ERR_UNSUPPORTED), dim <= 2048 (else UNSUPPORTED), a query dim other than the field's: NRTGPU_ERR_INVALID_ARG,
 * thread deadlines checked on entry and between passes (64 queries per pass), nrtgpu_knn_exact_bytes reports total_hits = live
 * docs that have a vector, nrtgpu_knn_exact_relation answers for byte fields too, forks share the rows, nrtgpu_get_stats counts
 * the passes in knn_panels / knn_rows / knn_score_launches / knn_score_ms.  A float entry point called on a byte field, and a
 * byte entry point on a float field, return NRTGPU_ERR_INVALID_ARG naming the field's element type.
 * A byte field as a RESCORER: nrtgpu_rescore_byte_vectors and nrtgpu_search_hybrid_bytes_batch below.
 * The request and the coalesced entries over a byte field: nrtgpu_knn_search_bytes_requests, nrtgpu_knn_search_bytes_coalesced and
 * nrtgpu_knn_exact_bytes_coalesced below.
 * Out of scope for byte fields (INVALID_ARG by that rule): the nrtgpu_dist_* entries -- and the float entries themselves, which
 * keep refusing a byte field: nrtgpu_knn_exact_coalesced, nrtgpu_knn_search_requests and nrtgpu_knn_search_coalesced are answered
 * for byte fields by their twins, not by a switch inside them; the Java shim does not bind the byte functions yet.
 * --------------------------------------------------------------------------------------------- */
int  nrtgpu_knn_exact_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                            int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                            float boost, nrtgpu_topdocs* out /* n_queries */);
int  nrtgpu_knn_search_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                             int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                             float boost, int32_t filter_mask, float min_score, nrtgpu_topdocs* out /* n_queries */);
/* knn requests over a BYTE field that share a pass although each has a pre-filter, threshold, k and boost of its OWN: the twins
 * of nrtgpu_knn_search_requests and nrtgpu_knn_search_coalesced (above), and of nrtgpu_knn_exact_coalesced.  A byte pass costs
 * the same for 1 query as for 64, and it is simpler than a float one: ONE pass returns final score bits -- no sketch, no
 * certificate, no second pass.
 * nrtgpu_knn_search_bytes_requests: query i gets exactly what
 * nrtgpu_knn_search_bytes(..., queries + i*dim, 1, dim, ks[i], boosts[i], filter_masks[i], min_scores[i], &out[i]) returns: same
 * docids, ranks, score bits, total_hits (= the hits returned; liveDocs always apply).  Passes of up to 64 queries at every
 * dimension, each searched with the largest k of its members and scores unboosted; member i takes the first ks[i] hits and its
 * own boost when the list is unpacked.  On the device a pass brings a table of accept sets (liveDocs & the member's filter, per
 * leaf and member) and the members' thresholds; a call whose requests are all equal is nrtgpu_knn_search_bytes itself, the
 * gather route (nrtgpu_set_knn_gather) included; requests that differ always pass over all rows.
 * Refusals, per request, are nrtgpu_knn_search_requests' with its wording ("query <i>: ..."): NRTGPU_ERR_INVALID_ARG for k <= 0,
 * filter_mask < 0, a min_score that is not >= 0, a boost that is not finite and > 0, a query dimension other than the field's,
 * ks == NULL; NRTGPU_ERR_UNSUPPORTED for k > NRTGPU_MAX_K, dim > 2048, a mask that is not resident on a leaf of the call that holds
 * the field's rows.  Two more, both NRTGPU_ERR_INVALID_ARG: a zero query under cosine ("query <i>: a zero vector ...") and a float
 * field (the error names the element type).  NULL boosts: all 1; NULL filter_masks: none; NULL min_scores: none.  A bad request
 * refuses the WHOLE call of the batch entry before anything is launched; in the coalesced entries it fails ALONE, before it is
 * queued.  Thread deadlines: checked on entry and between passes; NRTGPU_ERR_TIMEOUT for a request that expires in the queue.
 * nrtgpu_get_stats: a byte pass's counters -- knn_panels / knn_rows / knn_score_launches / knn_score_ms; nothing under
 * knn_sketch_launches or knn_second_passes.
 * nrtgpu_knn_search_bytes_coalesced / nrtgpu_knn_exact_bytes_coalesced: ONE request per call, blocking; the leave rule, the cohort
 * rule and the caps are the float entries' own.  Each has a queue of its own: float and byte callers never share a panel, nor do
 * the callers of the two byte entries.  nrtgpu_knn_exact_bytes_coalesced merges callers with one boost (finite, >= 0) and
 * answers as nrtgpu_knn_exact_bytes with n_queries = 1.
 * Out of scope: the nrtgpu_dist_* forms, the gather route for a pass whose members name different filters, MUST_NOT masks or
 * several filters per request, and the Java shim. */
int  nrtgpu_knn_search_bytes_requests(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim,
                                      const int32_t* ks, const float* boosts, const int32_t* filter_masks, const float* min_scores,
                                      nrtgpu_topdocs* out /* n_queries; out[i].capacity >= ks[i] */);
int  nrtgpu_knn_search_bytes_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                       int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, int32_t k, float boost,
                                       int32_t filter_mask, float min_score, nrtgpu_topdocs* out);
int  nrtgpu_knn_exact_bytes_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, int32_t k, float boost,
                                      nrtgpu_topdocs* out);
/* The GATHER route of the filtered knn entries.
 * Filtered knn requests (nrtgpu_knn_search, nrtgpu_knn_search_bytes; filter_mask != 0) whose filter accepts at most
 * max_accept_permille / 1000 of the field's rows over the call's leaves read ONLY the accepted rows. 0 (a context's default): never --
 * every request passes over all rows, as before.  Results are the same bits either way.
 * The share is judged on the host before anything is launched: per leaf that holds the field min(docs of the combined set
 * liveDocs & filter, rows of the field), summed -- an upper bound of the accepted rows (a sparse ord -> doc map accepts fewer) --
 * against max_accept_permille x the rows of those leaves; the accepted rows must also fit one candidate list of the full pass
 * (2^18 keys per query), else the full pass runs.  On the route the accepted rows are listed on the device once per call and every
 * pass of 64 queries scores exactly those with final score bits (float fields: the oracle's order of summation; byte fields: the
 * integers and the table above): no fp16 sketch is built or read, nothing is nominated, certified or passed over twice.  An
 * upper bound of 0 returns empty hit lists without a launch.  min_score, boost, total_hits, deadlines and every refusal are the
 * full pass's.  nrtgpu_get_stats: a pass counts as one knn_panels, adds the ACCEPTED rows to knn_rows and its scoring launch to
 * knn_score_launches / knn_score_ms, and nothing to knn_sketch_launches or knn_second_passes.
 * Out of scope: nrtgpu_knn_exact* (no filter argument), the coalesced and nrtgpu_dist_* entries, panels whose members have
 * different filters, keeping the row list from one call to the next, and a default other than 0. */
int  nrtgpu_set_knn_gather(nrtgpu_ctx* ctx, int32_t max_accept_permille);   /* 0..1000, else NRTGPU_ERR_INVALID_ARG */
/* The score of one (query, row) pair of a byte field from its three integers (the table above), exposed for the tests like
 * nrtgpu_fixed_point_scale: needs no device; it is the very function the kernel compiles.  Writes the UNBOOSTED score; returns 0,
 * or NRTGPU_ERR_INVALID_ARG (sim outside 0..3, dim outside 1..2048, integers `dim` int8 pairs cannot produce). */
int  nrtgpu_byte_vector_score(int32_t sim, int32_t dim, int32_t dot, int32_t q_norm2, int32_t v_norm2, float* out);

/* QueryRescore (rescore/QueryRescore.java:40-57) with a byte field's exact query (ExactByteVectorQuery, VectorFieldDef.java:842) in
 * the rescore slot: nrtgpu_rescore_vectors and nrtgpu_search_hybrid_batch (below) over a byte (int8) vector field.  query /
 * query_vectors: int8, `dim` per query.  The float entries keep refusing byte fields, and these refuse float fields.
 *   second pass  = (unboosted score of the table above) * boost, a float multiply: the bits nrtgpu_knn_exact_bytes returns for that
 *                  (query, row, boost); a zero row under cosine scores 0
 *   combined     = (float)(query_weight * (double)first + rescore_weight * (double)second)
 *   no vector    : a hit whose leaf lacks the field, or whose doc has no row, keeps (float)(query_weight * first)
 * Hits are re-sorted by (combined desc, doc asc) and trimmed to `window` (above NRTGPU_MAX_K: clamped, as the float entries do).
 * The two entries return the same bits: both kernels take the dot product -- an integer, exact in any order -- from one routine.
 * The rows are read where they lie, in the tiles of the search; a byte field has no second, row-major copy.
 * NRTGPU_ERR_INVALID_ARG: sim outside 0..3, a zero query under cosine, a query dim other than the field's, a float field (the message
 * names the element type), a boost that is not finite or < 0, and for nrtgpu_rescore_byte_vectors a hit outside every segment or
 * a weight that is not finite.  NRTGPU_ERR_UNSUPPORTED: dim > 2048, and for the hybrid entry a negative weight (the combined
 * scores are ranked on the device as keys that order like non-negative floats; nrtgpu_rescore_byte_vectors sorts on the host and
 * takes any finite weights).  Everything else of nrtgpu_search_hybrid_bytes_batch -- deadlines, content locks, the speculative
 * first pass with its re-run of tagged queries, statistics, total_hits and relation of the FIRST pass -- is
 * nrtgpu_search_hybrid_batch's: one code path. */
int  nrtgpu_rescore_byte_vectors(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                 int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, float boost,
                                 const int32_t* docs, const float* first_scores, int32_t n, double query_weight,
                                 double rescore_weight, int32_t window, nrtgpu_topdocs* out);
int  nrtgpu_search_hybrid_bytes_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t field_id, int32_t sim,
                                      const int8_t* query_vectors /* n_queries * dim */, int32_t dim, float boost,
                                      double query_weight, double rescore_weight, int32_t window, nrtgpu_topdocs* out /* n_queries */);

/* Vector rescorer: RescoreOperation.rescore(hits, ctx) of a QueryRescore whose rescoreQuery is an exact
 * vector query (src/main/java/com/yelp/nrtsearch/server/rescore/QueryRescore.java:40-57): every
 * first-pass hit gets combined = (float)(queryWeight * first + rescoreWeight * vectorScore) (double
 * arithmetic; hits without a vector keep queryWeight * first), hits are re-sorted by (score desc,
 * doc asc) and trimmed to `window`.  docs are global docids; doc_bases maps them to segments. */
int  nrtgpu_rescore_vectors(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                            int32_t field_id, int32_t sim, const float* query, int32_t dim, float boost,
                            const int32_t* docs, const float* first_scores, int32_t n, double query_weight,
                            double rescore_weight, int32_t window, nrtgpu_topdocs* out);

/* Hybrid tail (config C5): BM25 recall, then the vector rescorer over each query's hits, then the window --
 * on one stream, the first-pass hits never leave HBM (no host round trip between
 * SearchHandler.java:1412-1413 and RescoreTask.java:47-50).  Results are those of nrtgpu_search_bm25_batch
 * followed per query by nrtgpu_rescore_vectors(query_vectors[q]); total_hits / relation are the first
 * pass's (QueryRescorer keeps them).  Weights and boost must be >= 0 (else NRTGPU_ERR_UNSUPPORTED). */
int  nrtgpu_search_hybrid_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t field_id, int32_t sim,
                                const float* query_vectors /* n_queries * dim */, int32_t dim, float boost,
                                double query_weight, double rescore_weight, int32_t window,
                                nrtgpu_topdocs* out /* n_queries, capacity >= window */);

/* ---------------------------------------------------------------------------------------------
 * Function-score queries: MultiFunctionScoreQuery (src/main/java/com/yelp/nrtsearch/server/query/multifunction/
 * MultiFunctionScoreQuery.java) with WEIGHT functions over a BM25 disjunction -- "docs matching filter F score x 1.5".
 * The reference creates the inner weight with ScoreMode.COMPLETE and its scorer answers getMaxScore = Float.MAX_VALUE
 * (:168-174, :503-505): nothing is pruned, every live matching doc is scored, totalHits is exact.  So the inner query runs
 * exhaustively in a kernel of its own (csrc/funcscore.hip) that applies, per doc, between "sum of the clause scores" and
 * "key into the top-k" (MultiFunctionScoreQuery.java:445-500, WeightFilterFunction.java:66-71; one IEEE operation each):
 *   function score fs (double)   SCORE_MODE_MULTIPLY: 1.0, then for i = 0..n-1 in order, if the doc is in set i: fs *= (double)weight_i
 *                                SCORE_MODE_SUM:      0.0, fs += (double)weight_i for every matching i; none matched: fs = 1.0
 *   final score                  BOOST_MODE_MULTIPLY: (float)((double)inner * fs)   BOOST_MODE_SUM: (float)((double)inner + fs)
 *                                BOOST_MODE_REPLACE:  (float)fs                     n_functions == 0: inner itself (:449-451)
 *   hit test                     only when min_score > 0 or min_excluded (:334-336, :60-65): a doc is a hit iff
 *                                final > min_score || (!min_excluded && final == min_score); a doc that fails is no hit at all --
 *                                not counted in total_hits, not in the per-slice relation counts
 *   inner                        what nrtgpu_search_bm25 scores for the doc: (float) of the double sum of its matching clauses
 * queries[i] keeps its meaning for k, total_hits_threshold, has_after / after_* (searchAfter compares FINAL scores), filter_mask /
 * must_not_mask / more_* (the accept set restricts which docs match the inner query), liveDocs and slicing (nrtgpu_set_slicing,
 * nrtgpu_set_thread_slices).  total_hits is always the exact number of hits; total_hits_is_lower_bound follows the reference's
 * per-slice rule as on the exhaustive route; deadlines work as in nrtgpu_search_bm25_batch.
 * Refusals, each with a reason in nrtgpu_last_error:
 *   NRTGPU_ERR_INVALID_ARG  n_functions outside 0..NRTGPU_MAX_FUNCTIONS; modes outside their ranges; min_score < 0 or not finite;
 *                           a weight that is NaN, infinite or 0; functions == NULL with n_functions > 0; whatever
 *                           nrtgpu_search_bm25_batch refuses of queries[i] with that status
 *   NRTGPU_ERR_UNSUPPORTED  a weight < 0 (the reference may or may not throw at :454-460: the caller keeps Lucene); a function mask
 *                           that is not resident on a leaf of the call; an inner disjunction_max, any MUST clause,
 *                           min_should_match > 1 or min_competitive_score != 0; a batch whose queries do not all pass the
 *                           fixed-point analysis, or NRTGPU_FLAG_NO_FIXED_POINT (fixed-point sums are exact in any order, which
 *                           the kernel relies on); a context with NRTGPU_FLAG_PACKED_POSTINGS
 * The flat shapes refused here -- a DisjunctionMaxQuery, MUST clauses, min_should_match > 1 -- run as one group each under
 * nrtgpu_search_function_score_multi_match_batch (below).
 * Accounting: nrtgpu_last_diagnostics reports the call's items as items_scan (items_maxscore = 0); nrtgpu_get_stats counts the
 * launch under scan_launches, scan_items, scan_postings, scan_ms and fixed_point_launches.
 * Out of scope: script and decay functions (they read doc values); a match-all inner query; the coalesced, device-resident,
 * hybrid and nrtgpu_dist_* forms; pruning by the largest possible factor; the Java shim, which does not bind this yet.
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_FUNCTIONS 8
typedef struct {
  int32_t filter_mask;  /* 0: no filter query, the function applies to every doc; else a resident mask id (nrtgpu_segment_set_mask) */
  float   weight;       /* FilterFunction.getWeight(): finite, > 0.  The request's 0 means 1 (FilterFunction.java:83); the caller maps it */
} nrtgpu_score_function;                       /* 8 bytes */
typedef struct {
  int32_t n_functions;                         /* 0..NRTGPU_MAX_FUNCTIONS */
  const nrtgpu_score_function* functions;      /* in the request's order */
  int32_t score_mode;                          /* 0 SCORE_MODE_MULTIPLY, 1 SCORE_MODE_SUM */
  int32_t boost_mode;                          /* 0 BOOST_MODE_MULTIPLY, 1 BOOST_MODE_SUM, 2 BOOST_MODE_REPLACE */
  float   min_score;                           /* >= 0 */
  int32_t min_excluded;                        /* 0 / 1 */
} nrtgpu_function_score;                       /* 32 bytes */
/* n_queries function-score searches over the same leaves in one device pass; functions[i] wraps queries[i] */
int  nrtgpu_search_function_score_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                        const nrtgpu_bm25_query* queries, const nrtgpu_function_score* functions,
                                        int32_t n_queries, nrtgpu_topdocs* out);
/* The eligibility test alone, as nrtgpu_query_supported: NRTGPU_OK if the search above would run (q, fs) over these leaves, else
 * the status it would return with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_function_score_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                     const nrtgpu_function_score* fs);
/* The arithmetic above for one doc, exposed for the tests like nrtgpu_byte_vector_score: needs no device; it is the very function
 * the kernel compiles.  matched: bit i set = the doc is in function i's set.  Validates fs (the refusals above). */
int  nrtgpu_function_score_value(const nrtgpu_function_score* fs, uint32_t matched, float inner, float* out_score,
                                 int32_t* out_is_hit);

/* ---------------------------------------------------------------------------------------------
 * Multi-match queries: the TWO-LEVEL shapes the reference builds for a text search over several fields that analyses to
 * several tokens (multiMatchQuery, src/main/java/com/yelp/nrtsearch/server/query/QueryNodeMapper.java:429-528):
 *   best_fields  (:444-496)  a DisjunctionMaxQuery over one BooleanQuery of term clauses per field    NRTGPU_GROUPS_MAX_OF_SUM
 *   cross_fields (.../multimatch/MatchCrossFieldsQuery.java:163-192) a BooleanQuery with one clause per token, each a
 *                BlendedTermQuery, i.e. a DisjunctionMaxQuery of the token's per-field term queries     NRTGPU_GROUPS_SUM_OF_MAX
 * queries[i] holds ALL term clauses; groups[i] says which group (inner query) each belongs to.  The clauses run exhaustively in
 * a kernel of its own (csrc/multimatch.hip); nothing is pruned.  Per doc, c ranging over the clauses of a group that match it,
 * g over the groups that match it, groups and clauses in their order, every step one IEEE operation rounded once:
 *   dismax(max, sum)            (float)((double)max + (sum - (double)max) * (double)tie_breaker), sum the double sum of ALL scores:
 *                               DisjunctionMaxScorer's (float)(scoreMax + otherScoreSum * tieBreaker)
 *                               NRTGPU_GROUPS_SUM_OF_MAX                            NRTGPU_GROUPS_MAX_OF_SUM
 *   group g matches the doc     some clause of it does                              all SHOULD: >= max(1, group_min_should_match[g])
 *                                                                                   of its clauses do; all MUST: all of them do
 *   group score s_g             dismax(max_c score_c, sum_c (double)score_c)        (float) sum_c (double)score_c
 *   the doc is a hit            group_occur 0: >= max(1, min_should_match) groups   some group matches
 *                               match (more than n_groups: no hits, no error);
 *                               group_occur 1: every group matches
 *   score                       (float) sum_g (double)s_g                           dismax(max_g s_g, sum_g (double)s_g)
 * Everything else of queries[i] means what it means in nrtgpu_search_function_score_batch: k, total_hits_threshold, has_after /
 * after_* (searchAfter compares FINAL scores), filter_mask / must_not_mask / more_*, liveDocs, slicing, thread slices, deadlines.
 * total_hits is always exact; total_hits_is_lower_bound follows the per-slice rule of the exhaustive route.
 * Field boosts -- a BoostQuery around a per-field BooleanQuery, BlendedTermQuery's blended boosts -- are folded into the clauses'
 * `weight` by the caller, and so are the blended document frequencies of cross_fields (the caller takes them from the rewritten
 * query's TermStates: the library does not restate BlendedTermQuery.blend).
 * Refusals, each with a reason in nrtgpu_last_error:
 *   NRTGPU_ERR_INVALID_ARG  shape, n_groups, a group index or group_occur out of range; an empty group; a tie breaker outside 0..1
 *                           or not finite; a negative group minimum; group_of_term == NULL; queries[i].disjunction_max != 0 or
 *                           queries[i].tie_breaker != 0 (the structure lives in the groups); SUM_OF_MAX with any occur != 0;
 *                           MAX_OF_SUM with queries[i].min_should_match != 0 or group_occur != 0; whatever nrtgpu_search_bm25_batch
 *                           refuses of queries[i] with that status
 *   NRTGPU_ERR_UNSUPPORTED  a MAX_OF_SUM group that mixes MUST and SHOULD clauses; min_competitive_score != 0; a batch whose
 *                           queries do not all pass the fixed-point analysis, or NRTGPU_FLAG_NO_FIXED_POINT; a context with
 *                           NRTGPU_FLAG_PACKED_POSTINGS; a mask that is not resident; more than 4 scored fields or more than
 *                           NRTGPU_MAX_TERMS clauses
 * Accounting: as a function-score call (items_scan; scan_launches, scan_items, scan_postings, scan_ms, fixed_point_launches).
 * Out of scope: pruning (Lucene runs WAND here and reports a lower bound); MUST next to SHOULD inside a group; phrase-prefix,
 * fuzzy and synonym clauses; deeper nesting; the coalesced, device-resident, hybrid and nrtgpu_dist_* forms; packed postings;
 * the Java shim, which does not bind this yet.  (A function score over these shapes: the next section.)
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_GROUPS 8
#define NRTGPU_GROUPS_SUM_OF_MAX 0   /* BooleanQuery over DisjunctionMaxQuery groups: cross_fields */
#define NRTGPU_GROUPS_MAX_OF_SUM 1   /* DisjunctionMaxQuery over BooleanQuery groups: best_fields */
typedef struct {
  int32_t shape;
  int32_t n_groups;                      /* 1..NRTGPU_MAX_GROUPS; every group holds >= 1 clause */
  const int32_t* group_of_term;          /* queries[i].n_terms entries, 0..n_groups-1 */
  const int32_t* group_min_should_match; /* MAX_OF_SUM: n_groups entries, or NULL = all 0.  SUM_OF_MAX: not read */
  float   tie_breaker;                   /* of the DisjunctionMax level, 0..1 */
  int32_t group_occur;                   /* SUM_OF_MAX: 0 the groups are SHOULD clauses, 1 MUST.  MAX_OF_SUM: 0 */
} nrtgpu_clause_groups;                  /* 32 bytes */
/* n_queries multi-match searches over the same leaves in one device pass; groups[i] structures the clauses of queries[i] */
int  nrtgpu_search_multi_match_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                     const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries,
                                     nrtgpu_topdocs* out);
/* The eligibility test alone, as nrtgpu_query_supported: NRTGPU_OK if the search above would run (q, g) over these leaves, else
 * the status it would return with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_multi_match_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                  const nrtgpu_clause_groups* g);
/* The arithmetic above for one doc, exposed for the tests: needs no device; it calls the very functions the kernel compiles.
 * occur: n_terms entries of nrtgpu_term.occur, or NULL = all SHOULD; min_should_match: queries[i].min_should_match;
 * clause_scores: n_terms float scores; matched: bit t set = clause t matches the doc.  Validates g (the refusals above).
 * A doc that is no hit scores 0 when no group matches it, else what the groups that do match give. */
int  nrtgpu_multi_match_value(const nrtgpu_clause_groups* g, int32_t n_terms, const int32_t* occur, int32_t min_should_match,
                              const float* clause_scores, uint32_t matched, float* out_score, int32_t* out_is_hit);

/* ---------------------------------------------------------------------------------------------
 * A function score over a multi-match query: MultiFunctionScoreQuery wraps ANY inner Query (MultiFunctionScoreQuery.java:53,
 * :169-173, inner weight under ScoreMode.COMPLETE), and the text search a deployment sends is a multiMatchQuery wrapped in weight
 * functions.  The two sections above composed: queries[i] and groups[i] are a multi-match query, functions[i] wraps it.  One
 * kernel (csrc/multimatch.hip: bm25_multi_match_function_score_kernel) runs the clauses exhaustively; nothing is pruned.  Per doc:
 *   (inner, inner_hit)   the multi-match rule above, unchanged.  A doc with !inner_hit is no hit at all -- not counted in
 *                        total_hits, not in the per-slice relation counts -- whatever the functions say
 *   (final, hit)         the function-score rule above applied to inner, unchanged: function score, boost mode, the min_score
 *                        test.  n_functions == 0: final = inner, and the min_score test still applies
 * queries[i] means what it means in nrtgpu_search_multi_match_batch: k, total_hits_threshold, has_after / after_* (searchAfter
 * compares FINAL scores), filter_mask / must_not_mask / more_*, liveDocs, slicing, thread slices, deadlines.  total_hits is always
 * exact; total_hits_is_lower_bound follows the per-slice rule of the exhaustive route.
 * The grouping also expresses the flat shapes nrtgpu_search_function_score_batch refuses: a conjunction is one all-MUST
 * MAX_OF_SUM group, minimumNumberShouldMatch is one SHOULD MAX_OF_SUM group with a minimum, a flat DisjunctionMaxQuery with a
 * tie breaker is one SUM_OF_MAX group.
 * Refusals, each with a reason in nrtgpu_last_error, checked in this order:
 *   1. everything nrtgpu_search_multi_match_batch refuses of (queries[i], groups[i]), with its status, min_competitive_score != 0
 *      included
 *   2. everything nrtgpu_search_function_score_batch refuses of functions[i] alone, with its status (counts, modes, min_score,
 *      weights that are NaN, infinite, 0 or negative)
 *   3. NRTGPU_ERR_UNSUPPORTED  a context with NRTGPU_FLAG_PACKED_POSTINGS or NRTGPU_FLAG_NO_FIXED_POINT
 *   4. NRTGPU_ERR_UNSUPPORTED  a function mask that is not resident on a leaf of the call
 *   5. NRTGPU_ERR_UNSUPPORTED  what the planner refuses: a FILTER / MUST_NOT mask that is not resident, more than 4 scored fields,
 *      a batch whose queries do not all pass the fixed-point analysis
 * Accounting: as the two calls above (items_scan; scan_launches, scan_items, scan_postings, scan_ms, fixed_point_launches).
 * Out of scope: script and decay functions; pruning; the coalesced, device-resident, hybrid and nrtgpu_dist_* forms; packed
 * postings; the Java shim, which does not bind this yet.
 * --------------------------------------------------------------------------------------------- */
/* n_queries searches over the same leaves in one device pass; groups[i] structures the clauses of queries[i], functions[i] wraps it */
int  nrtgpu_search_function_score_multi_match_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                    const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups,
                                                    const nrtgpu_function_score* functions, int32_t n_queries, nrtgpu_topdocs* out);
/* The eligibility test alone, as nrtgpu_query_supported: NRTGPU_OK if the search above would run (q, g, fs) over these leaves, else
 * the status it would return with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_function_score_multi_match_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                                 const nrtgpu_clause_groups* g, const nrtgpu_function_score* fs);
/* The arithmetic above for one doc, exposed for the tests: needs no device; it calls the very functions the kernel compiles.
 * The first six arguments are nrtgpu_multi_match_value's (matched_clauses: bit t set = clause t matches the doc), then fs and
 * matched_functions as in nrtgpu_function_score_value (bit i set = the doc is in function i's set).  Validates g and fs (the
 * refusals above).  A doc the groups reject comes back with the inner score and *out_is_hit = 0. */
int  nrtgpu_function_score_multi_match_value(const nrtgpu_clause_groups* g, int32_t n_terms, const int32_t* occur, int32_t min_should_match,
                                             const float* clause_scores, uint32_t matched_clauses, const nrtgpu_function_score* fs,
                                             uint32_t matched_functions, float* out_score, int32_t* out_is_hit);

/* ---------------------------------------------------------------------------------------------
 * A text query beside knn clauses: a SearchRequest with `query` AND `knn`.  The reference resolves every knn query first -- each
 * becomes a doc-and-score query over its top k -- and ORs those into the main query as further SHOULD clauses of one BooleanQuery
 * (src/main/java/com/yelp/nrtsearch/server/search/SearchRequestProcessor.java:267-296, KnnUtils.resolveKnnQueryAndBoost).  The
 * lists are what nrtgpu_knn_search* returned; this entry scores the combined query in a kernel of its own
 * (csrc/knnclauses.hip: the function-score kernel's structure with a pass over the listed docs; nothing is pruned).
 * (nrtgpu_search_hybrid_batch is another thing: a rescorer tail that never admits a doc the text did not match.)
 * Score of a doc [Lucene-recall]; every operation is one IEEE operation:
 *   knn_sum   the double sum, in list order, of (double)(float)(scores[i] * boost) over the lists that hold the doc
 *   text      the doc's text clauses; they count only when the doc matches the text query AND lies in the query's accept set
 *             (liveDocs & FILTER & ~MUST_NOT)
 *   FLAT      text and lists: (float)(text_double_sum + knn_sum)     text only: what nrtgpu_search_bm25 scores
 *             lists only: (float)knn_sum
 *   NESTED    text and lists: (float)((double)(float)text_double_sum + knn_sum); the other two cases as FLAT
 * Which form: BooleanQuery.rewrite inlines a SHOULD clause that is itself a pure disjunction (all SHOULD,
 * minimumNumberShouldMatch <= 1) into the outer query, so a single term or a pure SHOULD disjunction is FLAT; a text query with
 * FILTER / MUST_NOT clauses is no pure disjunction and is NESTED.  text_nested == 0 with any mask set is NRTGPU_ERR_INVALID_ARG.
 * Hits: a doc is a hit if (the text matches and accepts it) or (it is in a list and live in its leaf).  A listed doc that is not
 * live is no hit; a listed doc outside the text's accept set is a hit with the lists' score alone.  k, has_after / after_*
 * (compares FINAL keys), total_hits_threshold, slicing, deadlines, total_hits (exact), the relation (per-slice rule), diagnostics
 * and statistics: as nrtgpu_search_function_score_batch.  n_lists == 0 is the text query alone.
 * Refusals, each with a reason in nrtgpu_last_error:
 *   NRTGPU_ERR_INVALID_ARG  n or n_lists out of range; NULL arrays with n > 0; a boost that is not finite or <= 0; a NaN or
 *                           infinite score; a doc twice in one list; a docid in no leaf of the call (or doc_bases == NULL with a
 *                           listed doc); text_nested outside 0..1, or 0 with a mask; whatever nrtgpu_search_bm25_batch refuses of
 *                           queries[i] with that status
 *   NRTGPU_ERR_UNSUPPORTED  a clause value <= 0 (the accumulators' 0 means "no match") or one that overflows; the exactness test
 *                           below fails; MUST clauses; disjunction_max; min_should_match > 1; min_competitive_score != 0; a
 *                           context with NRTGPU_FLAG_PACKED_POSTINGS or NRTGPU_FLAG_NO_FIXED_POINT; a batch that fails the
 *                           fixed-point analysis
 * Exactness test: sums are exact in any order, and the lists must keep that true.  With the clause values x = (float)(score *
 * boost): lo = min(-fx_E, min over x of floor(log2 x) - 23), hi = ceil(log2(sum of the text weights + sum over the lists of the
 * list's largest value)); hi - lo <= 53 is required (tiny scores beside BM25 scores are the only realistic trigger).  fx_E: the
 * largest nrtgpu_fixed_point_scale of the query's clauses that match anything; a query none of whose clauses matches anything is
 * tested over its lists alone.
 * Out of scope: the Java shim; the coalesced, device-resident and nrtgpu_dist_* forms; keeping the lists on the device between the
 * knn pass and this one; MUST / dismax / multi-match text under knn clauses; a function score on top; pruning; a request with
 * `knn` and no `query` (that is nrtgpu_knn_search*).
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_KNN_LISTS 8
typedef struct {            /* one resolved knn clause: what nrtgpu_knn_search* returned for it */
  const int32_t* docs;      /* global docids (doc_base + leaf doc), any order, no doc twice */
  const float*   scores;    /* the vector scores */
  int32_t n;                /* 0..NRTGPU_MAX_K */
  float   boost;            /* > 0, finite; the clause's value is (float)(scores[i] * boost), one float multiply
                               (DocAndScoreQuery under a BoostQuery); 1 when scores are already boosted */
} nrtgpu_doc_scores;        /* 24 bytes */
typedef struct {
  const nrtgpu_doc_scores* lists;
  int32_t n_lists;          /* 0..NRTGPU_MAX_KNN_LISTS */
  int32_t text_nested;      /* 0: the text clauses are clauses of the outer BooleanQuery (FLAT);
                               1: the text query is ONE clause whose float score is added (NESTED) */
} nrtgpu_knn_clauses;       /* 16 bytes */
/* n_queries text + knn searches over the same leaves in one device pass; knn[i] goes beside queries[i] */
int  nrtgpu_search_text_knn_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                  const nrtgpu_bm25_query* queries, const nrtgpu_knn_clauses* knn, int32_t n_queries,
                                  nrtgpu_topdocs* out);
/* The eligibility test alone: NRTGPU_OK if the search above would run (q, kc) over these leaves, else the status it would return
 * with the reason in nrtgpu_last_error ("a docid in no leaf of the call" aside: there are no doc_bases here).  No device work. */
int  nrtgpu_text_knn_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                               const nrtgpu_knn_clauses* kc);
/* The arithmetic above for one doc, exposed for the tests: needs no device; it is the very function the kernel compiles.
 * text_matched: the doc matches the text query and lies in its accept set; fixed_sum: its text clauses' sum x 2^fx_E as the
 * accumulators hold it; knn_sum: 0 = no list holds the doc. */
int  nrtgpu_text_knn_value(int32_t text_nested, int32_t text_matched, uint64_t fixed_sum, int32_t fx_E, double knn_sum, float* out);
/* The list checks and the exactness test above for one (q, kc) under the scale fx_E: 1 exact, 0 not, negative: the status the
 * search would return for the lists (of q only its clauses' weights and its masks are read).  Needs no device. */
int  nrtgpu_text_knn_exact(const nrtgpu_bm25_query* q, const nrtgpu_knn_clauses* kc, int32_t fx_E);

/* ---------------------------------------------------------------------------------------------
 * Sort by field: a text query's hits ordered by an int or float doc value column (nrtgpu_segment_add_doc_values) instead of by
 * score -- a request with a `querySort` (src/main/java/com/yelp/nrtsearch/server/search/SearchRequestProcessor.java:610 picks
 * search/collectors/SortFieldCollector.java:44-74: TopFieldCollectorManager(sort, topHits, searchAfter, totalHitsThreshold); the
 * sort from search/sort/SortParser.java:54-92 and field/NumberFieldDef.java:266-278).  ONE sort level over a 32-bit column.
 * Ranking is Sort(field) with Lucene's implicit docid tie break [Lucene-recall]: by value in the sort's direction (Integer.compare /
 * Float.compare: -0.0 < +0.0, NaN above +inf), equal values by global docid ascending whatever `reverse` is.  A doc with no value,
 * or in a leaf without the column, takes `missing_bits` as its value.  value_bits of a hit is the value it sorted as (for such a
 * doc the missing value, as in FieldDoc.fields; a NaN comes back as 0x7FC00000).
 * Matching: scores are not computed, only which docs match.  All clauses SHOULD: a doc is a hit iff at least
 * max(1, min_should_match) clauses match it (duplicate clauses count each); all clauses MUST: all of them match it.  The accept
 * set -- liveDocs, filter_mask / must_not_mask / more_* -- works as on the other routes.  The clauses' weights and norm caches
 * are not read for the result but must be valid: the queries are planned through the exhaustive plan.
 * Paging: the cursor lives in the sort (has_after, after_doc, after_bits: the last hit of the previous page); a hit is collected
 * iff it ranks strictly behind the cursor; hits of earlier pages still count in total_hits.  queries[i].has_after must be 0.
 * total_hits is always the exact number of hits; total_hits_is_lower_bound follows the reference's per-slice rule as on the
 * exhaustive route (some slice collected more than max(totalHitsThreshold, numHits) hits and numHits hits were returned), which
 * is TopFieldCollector's rule as well [Lucene-recall]; Lucene's own count under that flag is lower (it skips non-competitive
 * docs), ours is a valid value for GREATER_THAN_OR_EQUAL_TO.  Slicing, thread slices, deadlines, diagnostics (items_scan) and
 * statistics (scan_*, fixed_point_launches) work as in nrtgpu_search_function_score_batch.
 * Refusals, each with a reason in nrtgpu_last_error naming the query:
 *   NRTGPU_ERR_INVALID_ARG  NULL arguments; reverse or has_after outside 0..1; after_doc < 0; queries[i].has_after != 0; leaves of
 *                           the call that hold the field's column under different kinds or arities; whatever nrtgpu_search_bm25_batch
 *                           refuses of queries[i] with that status
 *   NRTGPU_ERR_UNSUPPORTED  the column is resident on no leaf of the call (its kind is then unknown), or it is MULTI-VALUED
 *                           (nrtgpu_segment_add_doc_values_multi: a sort names ONE value per doc -- upload the selector's pick
 *                           as a single-valued column of its own); disjunction_max != 0 or
 *                           tie_breaker != 0 (pass the clauses as a plain disjunction: scores are not read); MUST next to SHOULD
 *                           clauses; min_competitive_score != 0; k > NRTGPU_MAX_K; a mask that is not resident; a context with
 *                           NRTGPU_FLAG_PACKED_POSTINGS or NRTGPU_FLAG_NO_FIXED_POINT, a batch whose queries do not all pass
 *                           the fixed-point analysis -- the final-score routes' refusals, kept as they are: a KNOWN LIMIT, they
 *                           are stricter than a route that reads no score needs
 * 64-bit columns (LONG / DATE_TIME / DOUBLE, "newest first") are nrtgpu_search_sorted64_batch's, below; this entry refuses them.
 * Out of scope: STRING ordinals; LAT_LON distance; virtual (script) fields; more than one sort level; `score`
 * or `docid` as a sort level; scores beside the values; dismax / multi-match text under a sort (a match-all or filter-only query
 * under a sort is nrtgpu_search_docset_sorted_batch);
 * updatable doc values; the coalesced, device-resident and nrtgpu_dist_* forms; the Java shim, which does not bind this yet.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t  field_id;      /* the column */
  int32_t  reverse;       /* SortField.getReverse(): 0 ascending (smallest first), 1 descending */
  uint32_t missing_bits;  /* SortField.setMissingValue: what a doc without a value sorts AS, bits of the column's kind, taken
                           * verbatim (NumberFieldDef.java:275-276 passes MAX_VALUE / +inf for missingLast whatever `reverse` is:
                           * the caller does that mapping) */
  int32_t  has_after;     /* FieldDoc searchAfter (SortParser.parseLastHitInfo, :132-144) */
  int32_t  after_doc;     /* global docid */
  uint32_t after_bits;    /* the last hit's sort value */
} nrtgpu_field_sort;      /* 24 bytes */
typedef struct {          /* nrtgpu_topdocs with the hit's sort value where the score is (TopFieldCollector leaves score NaN) */
  int32_t   n_hits;                     /* out: hits written, <= k */
  int32_t   capacity;                   /* in : capacity of docs / value_bits (>= k) */
  int32_t*  docs;                       /* out: global docids, in the sort's order */
  uint32_t* value_bits;                 /* out: the value each hit sorted as, bits of the column's kind */
  int64_t   total_hits;                 /* out: live matching docs, exact */
  int32_t   total_hits_is_lower_bound;  /* out: 1 == GREATER_THAN_OR_EQUAL_TO (the per-slice rule above) */
} nrtgpu_fielddocs;
/* n_queries sorted searches over the same leaves in one device pass; sorts[i] orders queries[i] */
int  nrtgpu_search_sorted_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                const nrtgpu_bm25_query* queries, const nrtgpu_field_sort* sorts, int32_t n_queries,
                                nrtgpu_fielddocs* out);
/* The eligibility test alone: NRTGPU_OK if the search above would run (q, s) over these leaves, else the status it would return
 * with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_sorted_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                             const nrtgpu_field_sort* s);
/* The high word of the key a value sorts under (kind: NRTGPU_DOCVALUES_*), exposed for the tests: needs no device; it is the
 * very function the kernel compiles.  Larger = earlier in the sort's order.  kind or reverse outside 0..1: NRTGPU_ERR_INVALID_ARG. */
int  nrtgpu_sort_value_code(int32_t kind, int32_t reverse, uint32_t value_bits, uint32_t* out_key_high);

/* ---------------------------------------------------------------------------------------------
 * Sort by a 64-BIT field: "newest first" over a DATE_TIME column (epoch milliseconds as INT64: DateTimeFieldDef.getSortField,
 * src/main/java/com/yelp/nrtsearch/server/field/DateTimeFieldDef.java:108-125, sorts SortField.Type.LONG), ids, counters and
 * prices (LongFieldDef / DoubleFieldDef).  Semantics are nrtgpu_search_sorted_batch's, word for word, with 64-bit values and
 * Long.compare / Double.compare where it has Integer.compare / Float.compare [Lucene-recall]: matching (clause counts, MUST /
 * min_should_match, duplicates counting each, accept sets), the exact total_hits and the per-slice relation rule, slicing, thread
 * slices, deadlines, items_scan, scan_*; a doc without a value, or in a leaf without the column, sorts AS and reports
 * missing_bits (the reference's missing values are Long.MIN_VALUE / MAX_VALUE and -+inf: LongFieldDef.java:103-105,
 * DoubleFieldDef.java:105-107); EVERY NaN a sort reports is 0x7FF8000000000000, a column's and a NaN missing value's alike, whatever
 * its payload and whether or not the column holds a NaN (the 32-bit route's rule: its key holds the whole code).
 * The cursor (has_after, after_doc, after_bits) is tested
 * on values: a hit is collected iff (its value, its docid) ranks strictly behind (after_bits, after_doc) in the sort's order.
 * ONE PASS through the unchanged top-k: the keys stay 64 bits.  Per query, D is the maximum of doc_bases[i] + max_doc[i] over the
 * leaves, db = max(1, bit_length(D - 1)) the bits its global docids need, [lo, hi] the least and the greatest CODE of the sort's
 * column over the leaves of the call that hold a value (both the missing value's code if none does), span = hi - lo.  A key
 * packs the value's ordinal in that window -- 0 below lo, 1 + (code - lo) inside, span + 2 above hi; only the missing value can
 * lie outside -- above a db-bit docid field (nrtgpu_sort_key64).  THE SORT FITS iff span + 3 <= 2^(64 - db) - 1: with 10 M docs
 * 40 bits are left for values -- 34 years of milliseconds, any seconds column, any realistic id range.  A sort that does not fit
 * is refused with the reason, not widened.
 * The predicates have no doc_bases: they derive db from the leaves in order, with base 0 for the first (base[i + 1] = base[i] +
 * max_doc[i]); the batch entries use the caller's doc_bases (NULL: every leaf at base 0).  With the bases a searcher passes --
 * the leaves in order -- the two agree.
 * Refusals: nrtgpu_search_sorted_batch's table with the same statuses and precedence, and
 *   NRTGPU_ERR_INVALID_ARG  leaves that hold the field under different kinds
 *   NRTGPU_ERR_UNSUPPORTED  the column is resident on no leaf; it is a 32-bit or multi-valued column (the reason names
 *                           nrtgpu_search_sorted_batch); the sort does not fit -- the reason names the query, the field, the
 *                           bits the column's span needs and the bits the call's docids leave ("span needs 41 bits, 26-bit docids
 *                           leave 38"); a doc_bases[i] + max_doc[i] beyond 2^31
 * The text route keeps the final-score routes' flag and fixed-point refusals (the known limit).
 * Out of scope: DOUBLE columns whose values span more than the key leaves (two doubles of different sign do not fit, but for
 * -0.0 beside +0.0: a span of 1); a second sort level; terms counts over 64-bit columns; multi-valued 64-bit columns; the Java shim, which does not bind this yet.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t  field_id;      /* the column */
  int32_t  reverse;       /* 0 ascending, 1 descending */
  uint64_t missing_bits;  /* what a doc without a value sorts AS, bits of the column's kind: any value of the kind, inside the
                           * column's window or not; reported as given, a NaN as the canonical one */
  int32_t  has_after;     /* FieldDoc searchAfter */
  int32_t  after_doc;     /* global docid */
  uint64_t after_bits;    /* the last hit's sort value */
} nrtgpu_field_sort64;    /* 32 bytes */
typedef struct {
  int32_t   n_hits;                     /* out: hits written, <= k */
  int32_t   capacity;                   /* in : capacity of docs / value_bits (>= k) */
  int32_t*  docs;                       /* out: global docids, in the sort's order */
  uint64_t* value_bits;                 /* out: the value each hit sorted as, bits of the column's kind */
  int64_t   total_hits;                 /* out: live matching docs, exact */
  int32_t   total_hits_is_lower_bound;  /* out: 1 == GREATER_THAN_OR_EQUAL_TO (the per-slice rule) */
} nrtgpu_fielddocs64;                   /* 40 bytes */
int  nrtgpu_search_sorted64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                  const nrtgpu_bm25_query* queries, const nrtgpu_field_sort64* sorts, int32_t n_queries,
                                  nrtgpu_fielddocs64* out);
/* The eligibility test alone (db from the leaves in order, above).  No device work. */
int  nrtgpu_sorted64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                               const nrtgpu_field_sort64* s);
/* (The doc-set form, nrtgpu_search_docset_sorted64_batch, is declared with the doc-set requests below.) */
/* The key of one doc, exposed for the tests: needs no device; it is the very function the kernels compile.  (lo_bits, hi_bits):
 * the column's window as VALUES of the kind; has_value == 0: the doc sorts as missing_bits (value_bits is not read).  Larger =
 * earlier in the sort's order.  NRTGPU_ERR_UNSUPPORTED when (lo, hi, doc_bits) do not fit; NRTGPU_ERR_INVALID_ARG: out_key NULL,
 * kind outside 2..3, reverse / has_value outside 0..1, doc_bits outside 1..31, global_doc outside [0, 2^doc_bits), lo > hi in
 * the kind's order, a value outside [lo, hi].  The argument checks come first. */
int  nrtgpu_sort_key64(int32_t kind, int32_t reverse, uint64_t lo_bits, uint64_t hi_bits, uint64_t missing_bits, int32_t doc_bits,
                       int32_t has_value, uint64_t value_bits, int32_t global_doc, uint64_t* out_key);

/* ---------------------------------------------------------------------------------------------
 * Terms aggregation: a text query's hits counted per distinct value of an int or float doc value column
 * (nrtgpu_segment_add_doc_values) -- the per-hit half of a `TermsCollector` over a numeric field
 * (src/main/java/com/yelp/nrtsearch/server/search/collectors/additional/TermsCollectorManager.java;
 * IntTermsCollectorManager.java:142-152 and FloatTermsCollectorManager.java:149-150: countsMap.addTo(value, 1) for every
 * collected doc, ScoreMode.COMPLETE_NO_SCORES).  The call returns the WHOLE count map of each query; `size` and `BucketOrder`
 * (reduce(), TermsCollectorManager.java:430-483) stay with the caller, because the reference's own order among equal counts is
 * its hash map's iteration order and cannot be reproduced.  The call returns no hits: a request's top-k comes from whichever
 * search entry serves it, and the two calls are independent.
 * Which docs count: the sorted route's matching rule, word for word.  Scores are not computed, only which docs match.  All
 * clauses SHOULD: a doc is a hit iff at least max(1, min_should_match) clauses match it (duplicate clauses count each); all
 * clauses MUST: all of them match it.  Everything is tested inside the accept set -- liveDocs, filter_mask / must_not_mask /
 * more_*.  The clauses' weights and norm caches are not read for the result but must be valid: the queries are planned through
 * the exhaustive plan.  queries[i].k, has_after and totalHitsThreshold must be valid but are not read otherwise.
 * What is counted: a hit with a value adds 1 to the bucket of that value.  A hit without a value, or in a leaf that lacks the
 * column, adds to no bucket (docValues.size() == 0 in the reference).  total_hits counts every hit; hits_with_value is the sum
 * of all counts.
 * A MULTI-VALUED column (nrtgpu_segment_add_doc_values_multi): EVERY value instance of every hit adds 1 to its value's bucket
 * (for (i < docValues.size()) countsMap.addTo(docValues.get(i), 1), IntTermsCollectorManager.java:142-152; the float and the
 * ordinal collector alike, OrdinalTermsCollectorManager.java:189-226) -- a doc that holds a value twice counts it twice.
 * total_hits is unchanged; hits_with_value stays "the sum of all counts" and is then the number of value INSTANCES counted, which
 * may exceed total_hits.  Bucket identity, output order and overflowed ("distinct values > max_buckets") are as above.  A batch
 * may mix queries over columns of either arity.
 * Bucket identity is the identity of the column's code: ints are bucketed by value, floats by Float.floatToIntBits -- every NaN
 * falls in ONE bucket and reports as 0x7FC00000, -0.0 and +0.0 are TWO buckets (fastutil's Float2IntOpenHashMap equality
 * [Lucene-recall: never checked against a JVM run]).
 * Output order: buckets ascending in the kind's order (Integer.compare / Float.compare: -0.0 < +0.0, NaN above +inf), whatever
 * order the device filled its tables in.
 * Overflow: if the hits of a query hold MORE than max_buckets distinct values, the query reports overflowed = 1, n_buckets = 0
 * and hits_with_value = -1; its value_bits / counts are unspecified, its total_hits stays exact, the other queries of the batch
 * are unaffected; the caller sends that request to Lucene.  overflowed is exactly "distinct values > max_buckets".
 * Workspace bound (a design limit): a query's device table has the power of two >= 2 x max_buckets slots (at least 2); the
 * tables of ONE call may have 2^25 slots in all (256 MiB).  A batch of 256 queries may ask for the full 65536 buckets each.
 * Slicing, thread slices, deadlines, diagnostics (items_scan) and statistics (scan_*, fixed_point_launches) work as in
 * nrtgpu_search_sorted_batch.
 * Refusals, each with a reason in nrtgpu_last_error naming the query -- the sorted route's table, same statuses and precedence:
 *   NRTGPU_ERR_INVALID_ARG  NULL arguments; max_buckets outside 1..NRTGPU_MAX_TERM_BUCKETS; capacity < max_buckets, or NULL
 *                           value_bits / counts; leaves of the call that hold the field's column under different kinds, or
 *                           single-valued on one and multi-valued on another; whatever nrtgpu_search_bm25_batch refuses of
 *                           queries[i] with that status; a call whose tables
 *                           exceed the workspace bound above (the reason names the limit)
 *   NRTGPU_ERR_UNSUPPORTED  the column is resident on no leaf of the call; disjunction_max != 0 or tie_breaker != 0; MUST next
 *                           to SHOULD clauses; min_competitive_score != 0; k > NRTGPU_MAX_K; a mask that is not resident; a
 *                           context with NRTGPU_FLAG_PACKED_POSTINGS or NRTGPU_FLAG_NO_FIXED_POINT, a batch whose queries do
 *                           not all pass the fixed-point analysis -- the final-score routes' refusals, the KNOWN LIMIT they are
 *                           on the sorted route
 * A LONG / DATE_TIME / DOUBLE column is counted by nrtgpu_count_terms64_batch below.
 * Out of scope: string collectors as such (a string facet, SORTED_SET or single-valued, is uploaded as an
 * INT32 column of its global ordinals -- multi-valued where the field is -- and its keys mapped back by the caller); script and
 * virtual sources; nested collectors and NESTED_COLLECTOR order; the
 * Filter / Min / Max / Sum / TopHits collectors; fusing the count into a scoring route; dismax and multi-match text (a match-all
 * or filter-only query is nrtgpu_count_docset_terms_batch);
 * the coalesced, device-resident and nrtgpu_dist_* forms; the Java shim.
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_TERM_BUCKETS 65536
typedef struct {
  int32_t field_id;      /* the column, NRTGPU_DOCVALUES_INT32 or _FLOAT32 */
  int32_t max_buckets;   /* 1 .. NRTGPU_MAX_TERM_BUCKETS: more distinct values among the hits and the query overflows */
} nrtgpu_terms_count;    /* 8 bytes */
typedef struct {
  int32_t   n_buckets;        /* out: buckets written (0 when overflowed) */
  int32_t   capacity;         /* in : capacity of value_bits / counts, >= max_buckets */
  uint32_t* value_bits;       /* out: the buckets' values, bits of the column's kind, ascending in the kind's order */
  int32_t*  counts;           /* out: hits per bucket, each >= 1 */
  int64_t   total_hits;       /* out: live matching docs, exact */
  int64_t   hits_with_value;  /* out: the sum of counts; -1 when overflowed */
  int32_t   overflowed;       /* out: 1 == more than max_buckets distinct values */
  int32_t   reserved;         /* out: 0 */
} nrtgpu_term_counts;         /* 48 bytes */
/* n_queries count maps over the same leaves in one device pass; terms[i] names the column and the bound of queries[i] */
int  nrtgpu_count_terms_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                              const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms, int32_t n_queries,
                              nrtgpu_term_counts* out);
/* The eligibility test alone: NRTGPU_OK if the call above would run (q, t) over these leaves (with an output of sufficient
 * capacity), else the status it would return with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_count_terms_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                  const nrtgpu_terms_count* t);

/* ---------------------------------------------------------------------------------------------
 * Doc-set requests: a sort by field (nrtgpu_search_sorted_batch) or a terms count (nrtgpu_count_terms_batch) whose hit set is a
 * DOC SET and no text clause -- the reference's MatchAllDocsQuery, a BooleanQuery of FILTER / MUST_NOT clauses only, and the
 * numeric RangeQuery of an INT / FLOAT field with doc values, single- or multi-valued
 * (src/main/java/com/yelp/nrtsearch/server/field/IntFieldDef.java:124-160, FloatFieldDef.java:126-164:
 * IndexOrDocValuesQuery(PointRangeQuery, SortedNumericDocValuesField.newSlowRangeQuery)) under a `querySort` or a TermsCollector:
 * "everything in this category, rating between 4 and 5, best rated first", the facet counts of a browse page.
 * The hit set of docsets[i] is liveDocs AND every filter mask AND no must_not mask AND every range clause; with no mask and no
 * range it is every live doc.  filter_mask / must_not_mask / more_* have the meaning and the limits they have in
 * nrtgpu_bm25_query.
 * A range clause: both bounds are INCLUSIVE, bits of the column's kind (the kind is the resident column's).  The caller maps an
 * exclusive bound as the reference does (Math.addExact(+-1) for ints, FloatPoint.nextUp / nextDown for floats).  A doc passes iff
 * it HAS a value in the clause's column and lower <= value <= upper in the column's order [Lucene-recall]: Integer.compare for
 * ints; for floats the order of NumericUtils.floatToSortableInt(Float.floatToIntBits(.)) -- -0.0 < +0.0, every NaN the canonical
 * one and above +inf (so [NaN, NaN] keeps exactly the NaN docs, [-inf, +inf] drops them).  A doc without a value, or in a leaf
 * that lacks the column, fails the clause.  lower > upper in that order is an EMPTY range that matches nothing, not an error
 * (the reference's ensureUpperIsMoreThanLower is the caller's job).
 * A clause over a MULTI-VALUED column (nrtgpu_segment_add_doc_values_multi) keeps a doc iff SOME value of it passes that test
 * (SortedNumericDocValuesField.newSlowRangeQuery / IntPoint.newRangeQuery, IntFieldDef.java:124-158, FloatFieldDef.java:126-164);
 * a doc with no value fails.  A query may mix clauses over columns of either arity, and count or sort by a column of the other
 * arity; a count over a multi-valued column adds 1 per value instance (nrtgpu_count_terms_batch).  The SORT column must be
 * single-valued.
 * Results are nrtgpu_search_sorted_batch's and nrtgpu_count_terms_batch's, word for word, over this hit set: the order (value in
 * the sort's direction, ties by global docid ascending), the missing value, value_bits of a hit; paging (the cursor lives in the
 * sort, hits of earlier pages still count); the exact total_hits and the per-slice relation rule; bucket identity and ascending
 * output order; hits_with_value; overflowed exactly when the hits hold more than max_buckets distinct values, the other queries
 * of the batch unaffected; the 2^25-slot workspace bound.  total_hits_threshold enters the relation as on those routes.  Slicing,
 * thread slices, deadlines, diagnostics (items_scan) and statistics (scan_*) work as there; `postings` is 0: none is read.
 * Context flags: the route reads no posting and sums no score, so it RUNS under NRTGPU_FLAG_PACKED_POSTINGS and
 * NRTGPU_FLAG_NO_FIXED_POINT (the text routes over a doc value column refuse both).
 * Refusals, each with a reason in nrtgpu_last_error naming the query.  The predicates and the batch entries agree; all
 * NRTGPU_ERR_INVALID_ARG checks of ALL queries come before any NRTGPU_ERR_UNSUPPORTED one:
 *   NRTGPU_ERR_INVALID_ARG  NULL arguments; k outside 1..NRTGPU_MAX_K; total_hits_threshold < 0; n_ranges outside
 *                           0..NRTGPU_MAX_RANGES; ranges NULL with n_ranges > 0; a clause's reserved != 0; negative mask ids,
 *                           n_more_* negative or with a NULL array, more than NRTGPU_MAX_MASKS FILTER or MUST_NOT masks, a
 *                           more_* id <= 0; reserved != 0; what nrtgpu_search_sorted_batch / nrtgpu_count_terms_batch refuse of
 *                           sorts[i] / terms[i] / out[i] with this status; leaves of the call that hold a named column (the
 *                           sort's, the count's, a range clause's) under different kinds, or single-valued on one leaf and
 *                           multi-valued on another; a call whose count tables exceed the workspace bound
 *   NRTGPU_ERR_UNSUPPORTED  the sort or count column, or a range clause's column, is resident on no leaf of the call (its kind is
 *                           then unknown, and a forgotten upload must not read as "no hits"); a sort column that is multi-valued
 *                           (upload the selector's pick); a mask that is not resident
 * A sort by a LONG / DATE_TIME / DOUBLE column is nrtgpu_search_docset_sorted64_batch below, a count over one
 * nrtgpu_count_docset_terms64_batch; range clauses over such columns stay out of scope (a range over one is a built mask).  Out of scope: sorting by a multi-valued column; a score-ordered match-all; skipping whole
 * tiles by per-tile minima and maxima of a column (zone maps); the coalesced, device-resident and nrtgpu_dist_* forms; the Java
 * shim, which keeps sending these requests to Lucene until it binds this.  (A range, an in-set or an exists clause beside a text
 * query, a kNN query or any other route is a resident mask built from the column: nrtgpu_segment_set_mask_from_values.)
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_RANGES 4       /* range clauses per doc-set query (a design limit) */
typedef struct {
  int32_t  field_id;      /* the column, NRTGPU_DOCVALUES_INT32 or _FLOAT32 */
  uint32_t lower_bits;    /* inclusive, bits of the column's kind */
  uint32_t upper_bits;    /* inclusive */
  int32_t  reserved;      /* 0 */
} nrtgpu_range_clause;    /* 16 bytes */
typedef struct {
  int32_t filter_mask;              /* as in nrtgpu_bm25_query: 0 = none */
  int32_t must_not_mask;
  int32_t n_more_filters;
  int32_t n_more_must_not;
  const int32_t* more_filters;
  const int32_t* more_must_not;
  int32_t n_ranges;                 /* 0..NRTGPU_MAX_RANGES */
  int32_t k;                        /* numHits, 1..NRTGPU_MAX_K (a terms count reads it only to check it) */
  const nrtgpu_range_clause* ranges;
  int32_t total_hits_threshold;     /* >= 0; INT32_MAX: the count is never a lower bound */
  int32_t reserved;                 /* 0 */
} nrtgpu_docset_query;              /* 56 bytes */
/* n_queries sorted doc-set searches over the same leaves in one device pass; sorts[i] (cursor included) orders docsets[i] */
int  nrtgpu_search_docset_sorted_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                       const nrtgpu_docset_query* docsets, const nrtgpu_field_sort* sorts, int32_t n_queries,
                                       nrtgpu_fielddocs* out);
/* The eligibility test alone: NRTGPU_OK if the search above would run (d, s) over these leaves, else the status it would return
 * with the reason in nrtgpu_last_error.  No device work. */
int  nrtgpu_docset_sorted_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                    const nrtgpu_field_sort* s);
/* The sorted doc-set search over a 64-BIT sort column (nrtgpu_search_sorted64_batch: the packed key, the fit rule, the predicate's
 * doc bases): nrtgpu_search_docset_sorted_batch's semantics, word for word.  The doc set's own
 * `ranges` stay 32-bit clauses over 32-bit columns (a range over a 64-bit column is a mask built by
 * nrtgpu_segment_set_mask_from_values64, named as a filter).  Runs under both context flags, as its 32-bit form does. */
int  nrtgpu_search_docset_sorted64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                         const nrtgpu_docset_query* docsets, const nrtgpu_field_sort64* sorts, int32_t n_queries,
                                         nrtgpu_fielddocs64* out);
int  nrtgpu_docset_sorted64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs,
                                      const nrtgpu_docset_query* d, const nrtgpu_field_sort64* s);
/* n_queries count maps of doc sets over the same leaves in one device pass; terms[i] names the column and the bound of docsets[i] */
int  nrtgpu_count_docset_terms_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                     const nrtgpu_docset_query* docsets, const nrtgpu_terms_count* terms, int32_t n_queries,
                                     nrtgpu_term_counts* out);
/* The eligibility test alone (with an output of sufficient capacity).  No device work. */
int  nrtgpu_count_docset_terms_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                         const nrtgpu_terms_count* t);
/* Whether a range clause keeps a doc whose value is value_bits (kind: NRTGPU_DOCVALUES_*; *out = 1 / 0), exposed for the tests:
 * needs no device; it is the very function the kernels compile.  kind outside 0..1 or out NULL: NRTGPU_ERR_INVALID_ARG. */
int  nrtgpu_range_accepts(int32_t kind, uint32_t lower_bits, uint32_t upper_bits, uint32_t value_bits, int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * Terms aggregation over a 64-BIT column: a query's hits counted per distinct value of a LONG / DATE_TIME (epoch millis) /
 * DOUBLE doc value column (nrtgpu_segment_add_doc_values64) -- a facet on a business id, on a price stored as a double, on a day
 * bucket kept as a long.  The reference's TermsCollectorManager.buildManager (TermsCollectorManager.java:116-152) picks
 * LongTermsCollectorManager / DoubleTermsCollectorManager for such a field; their per-hit half is countsMap.addTo(value, 1) for
 * every value of every collected doc (LongTermsCollectorManager.java:145-148, DoubleTermsCollectorManager.java:147-150).
 * nrtgpu_count_terms64_batch is nrtgpu_count_terms_batch, and nrtgpu_count_docset_terms64_batch is
 * nrtgpu_count_docset_terms_batch, word for word over the same hit sets: the matching rule; a hit without a value, or in a leaf
 * that lacks the column, adds to no bucket; the exact total_hits; hits_with_value; overflowed exactly when the hits hold more than
 * max_buckets distinct values, the other queries of the batch unaffected; slicing, thread slices, deadlines, diagnostics and
 * statistics; the context flags each form runs under; the refusal tables with their statuses, and every NRTGPU_ERR_INVALID_ARG
 * check of ALL queries before any NRTGPU_ERR_UNSUPPORTED one.  nrtgpu_terms_count (field id, max_buckets in
 * 1..NRTGPU_MAX_TERM_BUCKETS) is reused as it is.  The count column is single-valued (no multi-valued 64-bit upload exists); the
 * doc set's own `ranges` stay 32-bit clauses over 32-bit columns of either arity.
 * Bucket identity is the identity of the column's code: LONG / DATE_TIME are bucketed by value, DOUBLE by
 * Double.doubleToLongBits -- every NaN, whatever its payload or sign, falls in ONE bucket and reports as 0x7FF8000000000000,
 * -0.0 and +0.0 are TWO buckets (fastutil's Double2IntOpenHashMap equality [Lucene-recall: never checked against a JVM run]).
 * Output order: buckets ascending in the kind's order (Long.compare / Double.compare: -0.0 < +0.0, NaN above +inf), whatever
 * order the device filled its tables in.  A batch may mix LONG and DOUBLE columns among its queries.
 * Every 64-bit pattern is a value here: Long.MIN_VALUE and Long.MAX_VALUE are buckets like any other.
 * Workspace bound (a design limit): a query's device table has the power of two >= 2 x max_buckets slots (at least 2); a slot
 * is 12 bytes (an 8-byte key and a 4-byte count), and the tables of ONE call keep the 32-bit entry's 256 MiB:
 * NRTGPU_TERMS64_MAX_CALL_SLOTS = 2^28 / 12 = 22369621 slots in all -- 170 queries may ask for the full 65536 buckets each.  A
 * call beyond it is NRTGPU_ERR_INVALID_ARG, the reason naming the limit.
 * Width refusals: these entries over a 32-bit column, single- or multi-valued, return NRTGPU_ERR_UNSUPPORTED with a reason that
 * names nrtgpu_count_terms_batch / nrtgpu_count_docset_terms_batch; the 32-bit entries over a 64-bit column keep refusing with
 * NRTGPU_ERR_UNSUPPORTED and now name these.
 * Out of scope: multi-valued 64-bit columns; range clauses over 64-bit columns inside a doc set (a built mask serves them);
 * nested collectors and NESTED_COLLECTOR order; script and virtual sources; the coalesced, device-resident and nrtgpu_dist_*
 * forms; the Java shim, which keeps sending these requests to Lucene.
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_TERMS64_LDS_SLOTS 8192              /* slots of a workgroup's LDS table (nrtgpu_terms_home_slots64) */
#define NRTGPU_TERMS64_MAX_CALL_SLOTS 22369621     /* table slots of one call, summed over its queries: 2^28 / 12 */
typedef struct {
  int32_t   n_buckets;        /* out: buckets written (0 when overflowed) */
  int32_t   capacity;         /* in : capacity of value_bits / counts, >= max_buckets */
  uint64_t* value_bits;       /* out: the buckets' values, bits of the column's kind, ascending in the kind's order */
  int32_t*  counts;           /* out: hits per bucket, each >= 1 */
  int64_t   total_hits;       /* out: live matching docs, exact */
  int64_t   hits_with_value;  /* out: the sum of counts; -1 when overflowed */
  int32_t   overflowed;       /* out: 1 == more than max_buckets distinct values */
  int32_t   reserved;         /* out: 0 */
} nrtgpu_term_counts64;       /* 48 bytes */
/* n_queries count maps over the same leaves in one device pass; terms[i] names the 64-bit column and the bound of queries[i] */
int  nrtgpu_count_terms64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms, int32_t n_queries,
                                nrtgpu_term_counts64* out);
/* The eligibility test alone (with an output of sufficient capacity).  No device work. */
int  nrtgpu_count_terms64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                    const nrtgpu_terms_count* t);
/* the same over doc sets */
int  nrtgpu_count_docset_terms64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                       const nrtgpu_docset_query* docsets, const nrtgpu_terms_count* terms, int32_t n_queries,
                                       nrtgpu_term_counts64* out);
int  nrtgpu_count_docset_terms64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                           const nrtgpu_terms_count* t);
/* The home slots of a value in the device's count tables, exposed for the tests: needs no device; it is the very function the
 * kernels compile.  *lds_slot: in a workgroup's table, below NRTGPU_TERMS64_LDS_SLOTS; *table_slot: in a query's table of
 * max_buckets, below the power of two >= 2 x max_buckets.  Probing from there is linear: 8 slots in the workgroup's table (then
 * the value goes to the query's table), the whole table in the query's.  The hash mixes both halves of the value's code.
 * kind outside 2..3, max_buckets outside 1..NRTGPU_MAX_TERM_BUCKETS or a NULL output: NRTGPU_ERR_INVALID_ARG. */
int  nrtgpu_terms_home_slots64(int32_t kind, uint64_t value_bits, int32_t max_buckets, uint32_t* lds_slot, uint32_t* table_slot);

/* ---------------------------------------------------------------------------------------------
 * Numeric range facets: a query's hits counted per requested value range of a single-valued doc value column -- "under 10,
 * 10-25, 25-50, over 50", "rated 4+, 3+, 2+", "added in the last day / week / month" (the last two overlap).  The reference's
 * Facet.numericRange (clientlib/src/main/proto/yelp/nrtsearch/search.proto:1285-1327), served by DrillSidewaysImpl.java:334-409:
 * INT and LONG fields become LongRange[] -> LongRangeFacetCounts, DOUBLE fields DoubleRange[] -> DoubleRangeFacetCounts.
 * Per query of a batch: a column and n_ranges (1..NRTGPU_MAX_COUNT_RANGES) ranges [lower, upper], BOTH bounds INCLUSIVE, bits
 * of the column's kind -- nrtgpu_range_clause's convention; the caller maps an exclusive bound (+-1, Math.nextUp / nextDown).
 * All four single-valued kinds are accepted: INT32, FLOAT32, INT64 (LONG, DATE_TIME), FLOAT64.  FLOAT32 has no counterpart in the
 * reference, which refuses FLOAT fields (DrillSidewaysImpl.java:367-371); the rule for it is the 32-bit range clause's order.
 * Which docs are hits.  nrtgpu_count_ranges_batch: nrtgpu_count_terms_batch's matching rule, word for word (all SHOULD: at least
 * max(1, min_should_match) clauses; all MUST: all of them; inside the accept set).  nrtgpu_count_docset_ranges_batch:
 * nrtgpu_count_docset_terms_batch's hit set, word for word (liveDocs, FILTER / MUST_NOT masks, the doc set's own 32-bit range
 * clauses over single- or multi-valued columns).
 * What is counted.  A hit that has a value v adds 1 to EVERY range with lower <= v <= upper in the column's code order: ints by
 * Integer.compare / Long.compare; floats and doubles in sortable-bits order -- -0.0 < +0.0, every NaN the canonical one and above
 * +inf.  Ranges may overlap, nest, repeat or touch; each is counted independently.  A hit without a value, or in a leaf that
 * lacks the column, adds to no range.  lower > upper in that order is an EMPTY range with count 0, not an error.
 * [Lucene-recall] a range facet counts a doc once per range that contains its value; DoubleRange compares through
 * NumericUtils.doubleToSortableLong; totCount is the number of hits that have a value.
 * Output per query: counts[n_ranges] in request order; total_hits, exact, with the per-slice relation machinery of the other
 * routes untouched; hits_with_value, the reference's totCount behind FacetResult.value.  topN, labels and the order of the
 * result stay with the caller.
 * How: the device counts per ELEMENTARY INTERVAL between the ranges' cut points (nrtgpu_range_cuts / nrtgpu_range_interval
 * below), the host sums the intervals a range covers -- exact integer sums; there is no bucket bound and no overflow state.
 * One call's queries must all name columns of ONE width: a batch that mixes 32- and 64-bit columns is NRTGPU_ERR_UNSUPPORTED
 * (split it).  The one entry serves both widths.
 * Context flags: the doc-set entry runs under NRTGPU_FLAG_PACKED_POSTINGS / NRTGPU_FLAG_NO_FIXED_POINT, the text entry refuses
 * both -- as their terms-count siblings do.  Slicing, thread slices, deadlines, diagnostics and statistics work as there.
 * Refusals, each with a reason in nrtgpu_last_error naming the query: the tables of nrtgpu_count_terms_batch /
 * nrtgpu_count_docset_terms_batch with the same statuses and precedence (max_buckets and the workspace bound aside); every
 * NRTGPU_ERR_INVALID_ARG check of EVERY query comes before any NRTGPU_ERR_UNSUPPORTED one; the predicates and the entries agree.
 * They add:
 *   NRTGPU_ERR_INVALID_ARG  n_ranges outside 1..NRTGPU_MAX_COUNT_RANGES; ranges NULL; a non-zero high word of a bound for a
 *                           32-bit kind; capacity < n_ranges or counts NULL; reserved != 0
 *   NRTGPU_ERR_UNSUPPORTED  a multi-valued count column (the reference counts a doc once per range there, which needs a per-doc
 *                           range mask instead of intervals); a batch that mixes 32- and 64-bit columns
 * Out of scope: multi-valued count columns; sampleTopDocs; facet scripts and virtual fields; drill-sideways per-dimension hit
 * sets (the call counts ONE hit set, the shim picks it); fusing the count into a scoring route; the coalesced, device-resident
 * and nrtgpu_dist_* forms; the Java shim, which keeps sending facet requests to Lucene until it binds this.
 * --------------------------------------------------------------------------------------------- */
#define NRTGPU_MAX_COUNT_RANGES 64
typedef struct {
  uint64_t lower_bits;    /* inclusive, bits of the column's kind; a 32-bit kind uses the low word, the high word is 0 */
  uint64_t upper_bits;    /* inclusive */
} nrtgpu_value_range;     /* 16 bytes */
typedef struct {
  int32_t field_id;       /* the column: a single-valued one of any NRTGPU_DOCVALUES_* kind */
  int32_t n_ranges;       /* 1 .. NRTGPU_MAX_COUNT_RANGES */
  const nrtgpu_value_range* ranges;
} nrtgpu_range_count;     /* 16 bytes */
typedef struct {
  int64_t* counts;           /* out: hits per range, in request order */
  int32_t  capacity;         /* in : capacity of counts, >= n_ranges */
  int32_t  reserved;         /* in : 0 */
  int64_t  total_hits;       /* out: live matching docs, exact */
  int64_t  hits_with_value;  /* out: hits that have a value in the column */
} nrtgpu_range_counts;       /* 32 bytes */
/* n_queries range facets over the same leaves in one device pass; ranges[i] names the column and the ranges of queries[i] */
int  nrtgpu_count_ranges_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                               const nrtgpu_bm25_query* queries, const nrtgpu_range_count* ranges, int32_t n_queries,
                               nrtgpu_range_counts* out);
/* The eligibility test alone (with an output of sufficient capacity).  No device work. */
int  nrtgpu_count_ranges_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                   const nrtgpu_range_count* r);
/* The same over doc sets: ranges[i] names the column and the ranges counted over the hits of docsets[i] */
int  nrtgpu_count_docset_ranges_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      const nrtgpu_docset_query* docsets, const nrtgpu_range_count* ranges, int32_t n_queries,
                                      nrtgpu_range_counts* out);
int  nrtgpu_count_docset_ranges_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                          const nrtgpu_range_count* r);
/* The cut points of a range list and the interval of a value, exposed for the tests: no device; they are the very functions the
 * host plans with and the kernels compile.  kind: NRTGPU_DOCVALUES_* (all four).
 * nrtgpu_range_cuts: the cuts of ranges[0 .. n_ranges), n_ranges in 0..NRTGPU_MAX_COUNT_RANGES, as CODES of the kind (a 32-bit
 * kind: in the low words), ascending without duplicates, into out_cuts[2 x NRTGPU_MAX_COUNT_RANGES]; *out_n_cuts of them.  Each
 * non-empty range gives its lower bound and the code behind its upper bound, the latter unless the upper bound is the kind's
 * greatest value.
 * nrtgpu_range_interval: the number of cuts[0 .. n_cuts) that are <= the code of value_bits, in 0..n_cuts; a range covers the
 * intervals from its lower bound's to its upper bound's.
 * NRTGPU_ERR_INVALID_ARG: a kind outside 0..3, NULL arguments, counts out of bounds, a non-zero high word for a 32-bit kind. */
int  nrtgpu_range_cuts(int32_t kind, const nrtgpu_value_range* ranges, int32_t n_ranges, uint64_t* out_cuts, int32_t* out_n_cuts);
int  nrtgpu_range_interval(int32_t kind, const uint64_t* cuts, int32_t n_cuts, uint64_t value_bits, int32_t* out_interval);

/* ---------------------------------------------------------------------------------------------
 * Host-side restatements the Java shim would otherwise take from Lucene objects
 * (BM25Similarity.scorer(boost, collectionStats, termStats); SmallFloat; slices()).
 * --------------------------------------------------------------------------------------------- */
/* The planner's fixed-point analysis of one clause, exposed for the tests: returns 1 and *out_scale = E when
 * every score the clause can produce over docs whose norm byte is <= max_norm -- weight - weight / (1 + freq *
 * norm_cache256[norm]), freq >= 1 -- is a positive integer below 2^32 after multiplication by 2^E (the
 * accumulators then add integers: exact, ds_add_u64); 0 when the range does not fit (the batch runs in fp64);
 * negative on bad arguments.  Needs no device. */
int  nrtgpu_fixed_point_scale(float weight, const float* norm_cache256, int32_t max_norm, int32_t* out_scale);
/* The planner's rule for cutting a batch's queries into work items (one item runs on one CU), exposed for the
 * tests: query_costs[q] = postings + 48 per 1024-doc sub-tile of the query (0: matches nothing), target_items =
 * CUs; out_items[q] = number of items.  Needs no device. */
int  nrtgpu_plan_item_counts(int32_t n_queries, const int64_t* query_costs, int32_t target_items, int64_t* out_items);
/* Multi-retriever blend (O(hits) host work, no device): BlenderOperation.blend =
 * mergeHits + sortAndPaginate (src/main/java/com/yelp/nrtsearch/server/search/multiretriever/blender/BlenderOperation.java:76-132).
 *   mode 0: WeightedRrfBlenderOperation (…/operation/WeightedRrfBlenderOperation.java:53-78): score = sum over retrievers, in
 *           declaration order, of boost / (rank_constant + rank), rank 1-based, float (…/score/WeightedRRFScoreDoc.java:62,75)
 *   mode 1: score order: score = sum of boost * the retriever's score
 * docs[r] / scores[r]: retriever r's hits in rank order (global docids), counts[r] of them; boosts NULL => 1.  Returns hits
 * [start_hit, top_hits) of the blended order; total_hits = distinct docs, relation GREATER_THAN_OR_EQUAL_TO as the
 * reference reports it.  Docs with EQUAL blended scores come out in the reference's order too: its java.util.HashMap
 * iteration order feeding a bounded java.util.PriorityQueue is restated (host_math.h). */
int  nrtgpu_blend(int32_t n_retrievers, const int32_t* const* docs, const float* const* scores, const int32_t* counts,
                  const float* boosts, int32_t mode, int32_t rank_constant, int32_t start_hit, int32_t top_hits, nrtgpu_topdocs* out);
int32_t nrtgpu_int_to_byte4(int32_t length);
int32_t nrtgpu_byte4_to_int(int32_t norm_byte);
float   nrtgpu_bm25_idf(int64_t doc_count, int64_t doc_freq);
float   nrtgpu_bm25_avgdl(int64_t sum_total_term_freq, int64_t doc_count);
void    nrtgpu_bm25_norm_cache(float avgdl, float k1, float b, float* out256);
/* MyIndexSearcher.slices / slicesForShards (src/main/java/com/yelp/nrtsearch/server/search/
 * MyIndexSearcher.java:79-208).  leaf i has max_docs[i] / num_docs[i] (live) docs and docBase
 * doc_bases[i].  Writes slice_of_leaf[i] = slice index (slices ordered as the reference orders
 * them) and returns the number of slices; with virtual_shards > 1 also writes shard_of_leaf[i]
 * (may be NULL). */
int32_t nrtgpu_slices(int32_t n_leaves, const int32_t* max_docs, const int32_t* num_docs, const int32_t* doc_bases,
                      int32_t virtual_shards, int32_t slice_max_docs, int32_t slice_max_segments,
                      int32_t* slice_of_leaf, int32_t* shard_of_leaf);

/* ---------------------------------------------------------------------------------------------
 * Deadlines and per-call diagnostics.
 * The reference checks the request's deadline between the phases of a search (src/main/java/com/yelp/nrtsearch/server/
 * handler/SearchHandler.java:158,194,263,277 -> grpc/DeadlineUtils.java:48-58) and bounds collection with timeoutSec
 * (search/SearchCutoffWrapper.java:149-159).  Here: the request thread states its deadline once -- absolute CLOCK_MONOTONIC
 * nanoseconds, 0 = none (the default) -- and every search / vector call it makes afterwards checks it on entry, again after
 * planning (i.e. after waiting for a workspace and for the device) and, in the vector search, between the passes over the
 * rows: past the deadline the call returns NRTGPU_ERR_TIMEOUT without launching (more) work.  A request waiting in
 * nrtgpu_search_bm25_coalesced carries its own thread's deadline: the batch leaves without it once it has expired.  Kernels
 * that are already launched run to completion (a batch is a few milliseconds); their results are returned as valid.
 * nrtgpu_last_diagnostics: what the calling thread's last completed search call cost -- the numbers behind
 * SearchResponse.Diagnostics.firstPassSearchTimeMs (SearchHandler.java:261) and a profile's per-phase times.
 * --------------------------------------------------------------------------------------------- */
void nrtgpu_set_thread_deadline_ns(int64_t deadline_ns);
int64_t nrtgpu_monotonic_ns(void);   /* the clock deadlines are on */
typedef struct {
  double  total_ms;        /* entry to return of the call (a coalesced request: of the batch it travelled in) */
  double  plan_ms;         /* host: queries -> launch plan */
  double  queue_ms;        /* waiting for a workspace and for the device (other batches' kernels) */
  double  device_ms;       /* scorer + merge kernels, HIP events; 0 unless nrtgpu_config.collect_timing */
  int64_t postings;        /* postings of the call's query terms (what an exhaustive scan streams) */
  int32_t queries;         /* queries of the batch */
  int32_t items_maxscore;  /* work items on the dynamic-pruning route */
  int32_t items_scan;      /* work items on the exhaustive route (a function-score call: all of its items) */
  int32_t reserved;
} nrtgpu_diagnostics;
int  nrtgpu_last_diagnostics(nrtgpu_diagnostics* out);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (maps onto SearchResponse.Diagnostics / profile fields).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batches;            /* batch calls completed */
  int64_t queries;
  int64_t scan_launches;      /* postings-scan kernel launches; a function-score call's kernel counts here, and in the four scan_* / fixed_point fields below */
  double  scan_ms;            /* sum of HIP-event durations of those launches (collect_timing) */
  int64_t scan_postings;      /* sum over launches of postings in the scanned term ranges */
  int64_t scan_items;
  double  merge_ms;
  double  host_plan_ms;       /* host time spent building launch plans */
  int64_t fixed_point_launches; /* scan launches that accumulated in exact fixed point (the others: fp64) */
  int64_t maxscore_launches;  /* launches of the MaxScore (dynamic pruning) kernel */
  double  maxscore_ms;        /* sum of their HIP-event durations (collect_timing) */
  int64_t maxscore_postings;  /* postings of the term ranges of the queries on that route (what an exhaustive scan streams) */
  int64_t maxscore_items;
  int64_t knn_panels;         /* exact vector searches: query panels (<= 32 queries) scored against every row */
  int64_t knn_score_launches; /* knn_score_kernel launches (a panel takes a few rounds, theta tightens in between) */
  double  knn_score_ms;       /* sum of their HIP-event durations (collect_timing) */
  int64_t knn_rows;           /* sum over panels of the rows scored */
  int64_t knn_second_passes;  /* panels that needed a second pass over the rows: a query's nominations did not certify its answer */
  int64_t knn_sketch_launches; /* of knn_score_launches: passes that nominated from the fp16 sketch (half the bytes per row) */
  int64_t spec_queries;       /* speculative thresholds (nrtgpu_set_speculation), since that call: queries run under them ... */
  int64_t spec_reruns;        /* ... queries whose guess failed the merge's check and were run again inside their call ... */
  int64_t spec_disabled;      /* ... 1 once the library has switched speculation off for one of the context's leaf sets: too many failed
                               * there even in the scattered order */
  int64_t spec_scattered;     /* ... 1 once a leaf set was moved to the scattered window order (its guesses failed in docid order: docids
                               * that are no sample of the index -- an index sort, time-ordered vocabulary) */
} nrtgpu_stats;
int  nrtgpu_get_stats(nrtgpu_ctx* ctx, nrtgpu_stats* out);
void nrtgpu_reset_stats(nrtgpu_ctx* ctx);
#ifdef __cplusplus
}
#endif
#endif /* NRTGPU_H */
