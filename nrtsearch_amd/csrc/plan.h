// plan.h -- launch-plan records shared by the host runtime and the gfx950 kernels.
// A "plan" is what one batch call uploads: per query, per (query, doc-range) work item, per
// (item, term) posting columns.  Names follow the reference's domain: leaves/segments, postings,
// slices (here: items), collectors.
#pragma once
#include <math.h>
#include <stdint.h>

namespace nrtgpu {

// Workgroup shape of the scan: waves x docs-per-sub-tile must fit 96 KiB of fp64 accumulators.
// 12 x 1024 (3 waves per SIMD, 168 VGPRs each) measured faster than 16 x 768 (4 per SIMD, 128 VGPRs:
// spills) on MI355X; a build-time choice (-DNRT_SCAN_WAVES / -DNRT_TILE_DOCS).
#ifndef NRT_SCAN_WAVES
#define NRT_SCAN_WAVES 12
#endif
#ifndef NRT_TILE_DOCS
#define NRT_TILE_DOCS 1024
#endif
constexpr int kTileDocs = NRT_TILE_DOCS;        // docs per wave-private LDS accumulator sub-tile (fp64)
constexpr int kScanWaves = NRT_SCAN_WAVES;      // autonomous wave64 per workgroup, 1 workgroup per CU (whole 160 KiB LDS)
constexpr int kScanThreads = kScanWaves * 64;
static_assert(kScanWaves % 4 == 0 && kTileDocs % 64 == 0 && kTileDocs / 64 <= 16, "scan workgroup shape");
static_assert(kScanWaves * kTileDocs * 8 <= 96 * 1024, "accumulators exceed their LDS share");
constexpr int kCandCap = (kScanWaves == 12) ? 1920 : 1664;  // scan: LDS candidate slots (what the LDS budget leaves next to four normInverse tables: 15 / 13 KiB; 2176 / 1920 with two tables measured the same)
constexpr int kMergeCap = 2048;     // merge: candidate slots = kMaxK + kScanThreads
constexpr int kLdsCaches = 4;       // normInverse tables kept in LDS per item (one per field)
// Score tables: for the kTabTerms densest terms of a query the BM25 score of every
// (freq <= kTabMaxFreq, norm byte < kTabNorms) pair is computed once per item into LDS, so scoring a
// posting is one LDS read.  Other (freq, norm) pairs / terms take the division path.
constexpr int kTabTerms = 5;
constexpr int kTabMaxFreq = 12;
constexpr int kTabNorms = 128;
constexpr int kTabEntries = (kTabMaxFreq + 1) * kTabNorms;  // row 0 (freq 0) unused
constexpr int kMaxK = 1024;
constexpr int kMaxTerms = 32;
// Packed postings (NRTGPU_FLAG_PACKED_POSTINGS): ONE 32-bit word per posting instead of the docid and
// code columns -- the doc's offset inside its 2^20-doc super-window (bits 12-31; the super-window is known from the
// posting's cell: cell shifts are capped so that a cell never spans two) | a 12-bit score code:
//   code <  kPackEscBase : (freq << 7) | norm byte (freq <= kTabMaxFreq, norm < kTabNorms): table byte offset = code << 2
//   code >= kPackEscBase : an EXCEPTION (freq > kTabMaxFreq or norm >= kTabNorms): the low 11 bits of its number e in
//                          the upload group's exception list (exceptions numbered in posting order).  The list's
//                          directory holds, per block of 2^kPackEscBlockShift = 2048 postings, the number of
//                          exceptions before the block (e0): e = e0 + ((low bits - e0) & 2047) -- unique, a block
//                          holds at most 2048.  exceptions[e] is the 32-bit escape word 0x80000000 | freq << 8 | norm
//                          of the unpacked layout.  Memory: 4 B per exception + 4 B per 2048 postings.
// The list (DTerm.fnorm of a packed term): u32 header[4] = {n_blocks, n_exceptions, 0, 0}, u32 dir[n_blocks + 1],
// u32 exceptions[n_exceptions].
// liveDocs are NOT folded into packed postings (no spare bit): deletes stay a mask the scorers test.
constexpr uint32_t kPackDocBits = 20;
constexpr uint32_t kPackCodeBits = 12;
constexpr uint32_t kPackCodeMask = (1u << kPackCodeBits) - 1u;
constexpr uint32_t kPackDocMask = (1u << kPackDocBits) - 1u;
constexpr uint32_t kPackEscBase = (uint32_t)kTabEntries;                    // 1664
constexpr uint32_t kPackEscBlockShift = 11;
constexpr uint32_t kPackEscLowMask = (1u << kPackEscBlockShift) - 1u;
static_assert(kPackEscBase + kPackEscLowMask < (1u << kPackCodeBits), "exception codes must fit the 12-bit code");
constexpr uint32_t kPackMaxCellShift = kPackDocBits - 10;                   // cell = tile >> shift with 1024-doc tiles: <= 2^20 docs
static_assert(kTileDocs == 1024 || kPackMaxCellShift > 0, "packed postings assume 1024-doc sub-tiles");

struct DTermAux;
// One query term inside one segment: where its posting columns live in HBM.
struct alignas(16) DTerm {
  const uint32_t* docids;    // docid column (all terms of the upload group, concatenated)
  const uint32_t* fnorm;     // score-code column: byte offset ((freq << 7 | norm) << 2) into a score table when
                             // freq <= kTabMaxFreq and norm < kTabNorms, else 0x80000000 | freq << 8 | norm.
                             // Packed postings: `docids` is the packed column and this is the group's exception list
  const uint32_t* cell_off;  // (n_cells + 1) posting offsets relative to `start`, one per doc-range cell
  uint64_t start;            // index of the term's first posting in the columns
  const DTermAux* aux;       // seal-time facts of the term the MaxScore route uses (resident next to the columns)
  uint32_t shift;            // cell = tile >> shift (0 for dense terms: one cell per tile)
  float    weight;           // boost * idf
  uint32_t cache_slot;       // per-query normInverse table index (< kLdsCaches)
  uint32_t tab_slot;         // bits 0-15: score table of this term in the item's LDS (< kTabTerms) or kTabSlotNone; bit 16: MUST clause
  int32_t  fx_scale;         // fixed-point batches: the term's scores are integers < 2^32 after * 2^fx_scale ...
  uint32_t fx_shift;         // ... and enter the query's common scale 2^-fx_E shifted left by fx_shift
};
static_assert(sizeof(DTerm) == 64, "DTerm layout");

// The host uploads a COMPACT plan: per query clause one DQTerm naming the term's resident per-leaf table (the static
// half of a DTerm for every leaf of the leaf set, written once per term: planner.cpp, LeafSetCache) plus the query's
// side of it; expand_terms_kernel writes the DTerm records of every (query, leaf) the scorers read.  The host touches
// one cache line per clause instead of one per (clause, leaf).
struct alignas(16) DQTerm {
  const DTerm* table;        // n_leaves entries; docids == nullptr: the leaf lacks the term; `weight` holds the posting count (bits)
  float    weight;           // boost * idf
  uint32_t cache_slot;
  uint32_t tab_slot;
  int32_t  fx_scale;
  uint32_t fx_shift;
  uint32_t pad;
};
static_assert(sizeof(DQTerm) == 32, "DQTerm layout");
struct alignas(16) DQExpand {
  uint32_t term_begin;       // the query's DQTerms
  uint32_t n_terms;
  uint32_t by_weight;        // order of a (query, leaf)'s DTerms: 1 = heaviest clause first (MaxScore route), 0 = densest first
  uint32_t cache_off;        // offset in floats of the query's first normInverse table (DItem.cache_off): the walk rows' bounds
};
static_assert(sizeof(DQExpand) == 16, "DQExpand layout");
// What the expansion needs for the MaxScore route's walk rows (DWalkRow, below): ONE record in the plan upload, directly in front
// of the batch's DQExpand array (expand_terms_kernel reads it in front of qx[0]; its arguments stay the compact plan's).
struct DWalkRow;
struct DQuery;
struct alignas(16) DExpandHead {
  const float* caches;       // the queries' normInverse tables (DQExpand.cache_off indexes them)
  const DQuery* queries;     // DQuery.combine_max: suffix maxima instead of sums
  DWalkRow* rows;            // one row per DTerm of a by_weight query, same index; nullptr: none are written
  uint64_t pad;
};
static_assert(sizeof(DExpandHead) == 2 * sizeof(DQExpand), "the head takes the place of two DQExpand records");

// What the MaxScore route (maxscore.hip) knows about a term besides its columns (one record per term of a segment,
// written at seal): the term's impact frontier -- per freq the smallest norm byte it occurs with -- from which the kernel
// takes the term's exact maximum score under the query's statistics (the role of Lucene's competitive (freq, norm) impacts,
// SURVEY 8a row a5) -- and a doc -> posting LOOKUP structure for the walk's later clauses:
//   kLookBits  : MEMBERSHIP + RANK RECORDS, per 32 docs {doc bits, postings of the term before the block}: whether the doc is
//                there and where its posting is; its score code is a second, dependent gather.  0.25 B per doc -- 16 KB per
//                65 536-doc window, and 2.5 MB for a whole 10 M-doc segment: the records of the terms that hundreds of a
//                batch's queries share stay in L2 / the Infinity Cache.
//   kLookCells : LOOKUP CELLS, one posting offset per 2^look_shift docs with look_shift chosen so that a cell holds
//                0.5 - 1 posting on average (4 - 8 B per POSTING): a search in the doc's cell, usually over no posting or one.
//   kLookNone  : the doc is searched for in its cell of the tile-granular table DTerm.cell_off (~4 - 8 postings per cell).
// Which term gets what: segment.cpp: build_term_aux (the segment's lookup budget, nrtgpu_config.lookup_budget_pct).
// Measured and dropped (round 5, profiles/r05_look_policy_matrix.log; kernel ms per 1024 C3 queries, same box): structures that
// answer in ONE gather instead of two -- a 16-bit code map per doc (2 B per doc) 2.97, a 4-bit freq map + the field's norm bytes
// (0.5 B per doc) 3.56 -- against 2.11 for the records: what a lookup costs is decided by how much of the structure the caches
// hold (a map of a frequent term is 8x / 2x the records plus nothing saved on the absent docs, the common answer), not by the
// number of dependent gathers.  No structure at all: 6.72; lookup cells for every term: 3.20.
// Deleted docs need no care here: a doc whose postings were re-coded to score 0 (apply_live_kernel) never survives the stream
// phase of the walk, so it is never looked up.
constexpr uint32_t kLookNone = 0, kLookBits = 1, kLookCells = 2;
struct alignas(16) DTermAux {
  const void* look;        // the records (uint32_t[2][max_doc / 32 + pad]) / the lookup cells (uint32_t[cells + 1], offsets
                           // relative to the term's first posting); nullptr: kLookNone
  uint8_t  min_norm[12];   // postings a score table can serve (freq f = 1..12, norm byte < 128): smallest norm byte
                           // seen with freq f at [f - 1]; 0xFF = no such posting
  uint8_t  esc_min_norm;   // the other postings (freq > 12 or norm byte >= 128): smallest norm byte ...
  uint8_t  look_kind;      // kLook*
  uint8_t  look_shift;     // kLookCells: log2 of the docs per cell
  uint8_t  pad;
  uint32_t esc_max_freq;   // ... and largest freq among them; 0 = none
  uint32_t pad2;
};
static_assert(sizeof(DTermAux) == 32, "DTermAux layout");

// WALK ROWS: what the MaxScore walk needs of a clause that depends only on (query, leaf) -- the part-static image of the record
// a wave keeps per clause in LDS (maxscore.hip: WClause, the same 80 bytes) with the clause's bounds filled in: its exact maximum
// score in the leaf under the query's statistics, ub, from the term's impact frontier (DTermAux), what the clauses after it can add
// (sum; DisjunctionMaxQuery: lift a doc to, the maximum), u_after = S_{c+1}, and suffix = S_c.  expand_terms_kernel writes one row
// next to every DTerm of a query on that route (same index, out_begin + rank), once per (query, leaf); a wave that enters a part
// copies the part's rows into its LDS table instead of working them out again -- an item's 12 waves and its helpers all did.
struct alignas(16) DWalkRow {
  uint64_t docids, fnorm;   // column bases
  uint64_t suffix;          // S_c = ub combined with u_after (the walk keeps a window's posting range in these two slots)
  uint64_t ub;              // the clause's maximum score in the leaf, in the query's common fixed-point scale
  float    weight;
  int32_t  fx_scale;
  uint32_t flags;           // as WClause.flags; the MUST bit is filled whatever kernel variant reads the row
  uint32_t pad;
  uint64_t u_after;
  uint64_t look;            // DTermAux.look, 0 = none
  uint64_t cells, start;    // DTerm.cell_off, DTerm.start
};
static_assert(sizeof(DWalkRow) == 80, "DWalkRow layout");
// the flags word of a walk row / WClause (maxscore.hip documents the fields)
__host__ __device__ inline uint32_t walk_row_flags(uint32_t tab_slot, uint32_t fx_shift, uint32_t cache_slot, uint32_t cell_shift,
                                                   uint32_t look_kind, uint32_t look_shift, bool must) {
  return ((tab_slot & 0xFFFFu) < (uint32_t)kTabTerms ? (tab_slot & 0xFFFFu) : 7u) | (must ? 8u : 0u) | (fx_shift << 4) | (cache_slot << 8) |
         ((cell_shift & 31u) << 16) | ((look_kind & 7u) << 24) | ((look_shift & 31u) << 27);
}

// Workgroup shape of the MaxScore route: 12 autonomous waves (168 VGPRs each); a wave owns a window of kMsWinTiles
// sub-tiles at a time (its docs' "already evaluated" bits: kMsWinDocs / 8 bytes of LDS).
#ifndef NRT_MS_WIN_TILES
#define NRT_MS_WIN_TILES 64
#endif
#ifndef NRT_MS_WAVES
#define NRT_MS_WAVES 12
#endif
#ifndef NRT_MS_SLOTS
#define NRT_MS_SLOTS 8
#endif
constexpr int kMsWaves = NRT_MS_WAVES;
constexpr int kMsSlots = NRT_MS_SLOTS;   // postings per lane and instruction: 8 (two 16-byte loads per column) or 4
static_assert(kMsSlots == 4 || kMsSlots == 8, "MaxScore kernel: 4 or 8 postings per lane");
constexpr int kMsThreads = kMsWaves * 64;
static_assert(kMsThreads <= 1024, "a workgroup holds at most 16 waves");
constexpr int kMsWinTiles = NRT_MS_WIN_TILES;
constexpr int kMsWinDocs = kMsWinTiles * kTileDocs;
constexpr int kMsMaxTerms = 8;      // clauses of a query on the MaxScore route (longer disjunctions are scanned exhaustively)
// A query whose hit count is not certain to pass the threshold (or that wants the exact count: ScoreMode.COMPLETE) may still
// run in the MaxScore kernel when it is SMALL (<= this many postings over all clauses and leaves): in EXACT mode the kernel
// skips nothing, so every matching doc is evaluated once and counted -- the exhaustive scan's answer, without walking every
// 1024-doc sub-tile of the shard for a handful of postings.
constexpr int64_t kMsExactMaxPostings = 1 << 18;
#ifndef NRT_MS_CAND_CAP
#define NRT_MS_CAND_CAP (NRT_MS_WIN_TILES > 32 ? 2304 : 3072)
#endif
constexpr int kMsCandCap = NRT_MS_CAND_CAP;  // LDS candidate slots (>= kMaxK + 512: a wave's retry always fits)
static_assert(kMsCandCap >= kMaxK + 512, "candidate buffer too small");
// item_hits of a MaxScore item: the docs it evaluated, plus kHitsPrunedUnit when it skipped anything (the count is
// then a lower bound).  The merge kernel's plain sum keeps both: low 48 bits = docs, high 16 = pruned items.
constexpr uint64_t kHitsPrunedUnit = 1ull << 48;
// Speculative thresholds (maxscore.hip: "speculation"; search.cpp: the re-run): a workgroup that has walked a fraction g of a
// query's doc windows holds the exact top-k of THOSE docs; if docs are spread over windows like a random sample, about k x g of
// the query's final top-k lie among them, so the (k g + z sqrt(k g))-th best key it holds is -- z standard deviations deep --
// below the final k-th key, and a far better theta than the k-th best of the docs seen so far.  It is a GUESS: everything it
// skips is only known to score below the guess.  The merge therefore checks it -- the merged list's k-th key must reach the
// largest guess published for the query (then nothing skipped could have entered) -- and tags the query's count with
// kHitsSpecInvalid otherwise; the host runs tagged queries again without speculation.  The results are exact either way.
constexpr uint64_t kHitsSpecInvalid = 1ull << 47;

// One part of a work item: a contiguous tile range of one segment (a LeafReaderContextPartition).
struct alignas(16) DPart {
  const uint64_t* live_bits;  // nullptr => every doc live
  uint32_t term_begin;        // first DTerm of (query, segment); terms sorted by postings, densest first
  uint32_t n_terms;
  uint32_t tile_begin, tile_end;
  uint32_t max_doc;
  int32_t  doc_base;
  uint32_t tile_offset;       // sub-tiles of the item's earlier parts: the item's sub-tiles form one sequence
  uint32_t slice;             // bits 0-23: the searcher slice (MyIndexSearcher.slices) the part's leaf belongs to, an index into the
                              // query's per-slice hit sums (DQuery.slice_base); bits 24-31: the slice's slot among the item's
                              // slices (< kSliceSlots): the item counts its hits per slot
};
static_assert(sizeof(DPart) == 48, "DPart layout");

// One work item == one workgroup == one collector: a query over a list of parts visited in docBase
// order, sharing one candidate buffer / theta -- the analogue of a Lucene LeafSlice
// (/root/reference/src/main/java/com/yelp/nrtsearch/server/search/MyIndexSearcher.java:163-208).
struct alignas(16) DItem {
  uint32_t query;             // batch-local query index
  uint32_t part_begin;
  uint32_t n_parts;
  uint32_t cache_off;         // offset in floats of the query's first normInverse table
  uint32_t n_caches;
  uint32_t n_tabs;            // score tables to build (<= kTabTerms)
  float    tab_weight[kTabTerms];
  uint32_t tab_cache[kTabTerms];  // normInverse table of each score table
  int32_t  tab_scale[kTabTerms];  // fixed-point batches: fx_scale of each score table's term
  int32_t  fx_E;                  // fixed-point batches: accumulators hold score * 2^fx_E
  uint32_t peer_slot;             // this item's slot among the query's items [DQuery.item_begin, + n_items)
  uint32_t flags;                 // MaxScore kernel, bits 0-1: when bounds may skip work (kMsMode*); bits 2-3: the item's doc windows hold
                                  // kMsWinTiles >> that many sub-tiles (planner.cpp: the launch's heaviest queries get finer ones);
                                  // bits 8-31: the item's doc windows (summed over its parts): what helpers share with the owner
};
static_assert(sizeof(DItem) == 96, "DItem layout");

struct alignas(16) DQuery {
  uint32_t k;
  uint32_t has_after;
  int32_t  after_doc;      // global docid
  float    after_score;
  uint32_t item_begin;     // items of this query are [item_begin, item_begin + n_items)
  uint32_t n_items;
  uint32_t min_should_match;  // > 1: only docs matched by that many clauses are hits (count-carrying kernel variant)
  uint32_t combine_max;       // 1: DisjunctionMaxQuery (tie breaker 0): a doc scores its best clause, not the sum (same variant)
  uint32_t gte_floor;         // max(totalHitsThreshold, numHits): a slice that collects more hits makes the relation
                              // GREATER_THAN_OR_EQUAL_TO (LazyQueueTopScoreDocCollector.java:176-199); ~0: never (ScoreMode.COMPLETE)
  uint32_t slice_base;        // the query's per-slice hit sums: slice_sum[slice_base + slice]
  uint32_t sec_mode;          // MaxScore kernel, SHAPES == 2: the doc's score needs a SECOND accumulator next to the sum (kMsSec*)
  float    tie_breaker;       // kMsSecTieBreaker: DisjunctionMaxQuery.tieBreakerMultiplier
};
static_assert(sizeof(DQuery) == 48, "DQuery layout");
// Hit counting (both scorers): an item counts the live matching docs of each searcher slice it touches (at most kSliceSlots
// of them: the planner cuts items there) in LDS and adds them to the query's per-slice sums at its end; slice_relation_kernel
// then applies the reference's rule -- one collector per slice, MyIndexSearcher.java:163-208 -- to the sums.
constexpr int kSliceSlots = 8;
// MaxScore kernel, DItem.flags bits 0-1: when may bounds skip work?
//   kMsModePrune : from the start (the planner KNOWS some slice passes max(totalHitsThreshold, numHits): what is reported is
//                  its certain lower bound)
//   kMsModeExact : never (ScoreMode.COMPLETE on a small query): every live matching doc is evaluated and counted
//   kMsModeCount : like Lucene's collector (LazyQueueTopScoreDocCollector.java:176-199: no min competitive score before
//                  totalHits has passed the threshold) -- exact counting until some slice's count passes gte_floor, from
//                  then on bounds skip and the count is a lower bound (relation GREATER_THAN_OR_EQUAL_TO)
constexpr uint32_t kMsModePrune = 0, kMsModeExact = 1, kMsModeCount = 2;
// DQuery.sec_mode: scores that are not ONE sum of the matching clauses' scores.  The walk's bounds stay bounds of the plain sum
// (either score is at most what the sum scores, up to the float rounding kMsSecReqOpt's threshold allows for); the second
// accumulator only enters the final key.
//   kMsSecTieBreaker : DisjunctionMaxQuery with a tie breaker > 0: second = the best clause; score = (float)(best + (sum - best) * tb)
//   kMsSecReqOpt     : MUST next to SHOULD clauses: second = the sum of the SHOULD clauses; score = (float)(sum - second) + (float)second;
//                      a doc that lacks a MUST clause (DTerm.tab_slot bit 16) is no hit
constexpr uint32_t kMsSecNone = 0, kMsSecTieBreaker = 1, kMsSecReqOpt = 2;
// DTerm.tab_slot: bits 0-15 the score table (0xFFFF: none), bit 16: a MUST clause
constexpr uint32_t kTabSlotNone = 0xFFFFu, kTabSlotRequired = 1u << 16;
// minimumNumberShouldMatch > 1: the fixed-point accumulator carries the number of matching clauses above
// the score sum (sum < 2^52: 32 clauses x 2^32 x 2^15)
constexpr int kMsmCountShift = 56;

// Helping (maxscore.hip): the windows of an item are handed out by a counter in GLOBAL memory, so a workgroup other than the
// item's own -- a HELPER -- can take windows of an item that is running.  The launch has n_own + n_help workgroups; the items
// themselves are a queue in launch order (item_next).  A workgroup that gets a CU starts the next item, or helps: an item on
// the launch's critical path while the queue still holds items, any unfinished item once it is empty -- the tail of a launch
// (1024 items of very different cost on 256 CUs, one workgroup per CU) is shared instead of waited for.  A helper has its own
// score tables, candidate list and output slot (slot_base + its number), starts from the theta the query's items have
// published (theta_g) and notes its query beside its slot (help_query) for the merge.
struct DHelp {
  uint32_t* win_next;            // [n_own]   windows handed out beyond the owner's first kMsWaves (zeroed per launch)
  uint32_t* help_cnt;            // [n_own]   helpers that joined the item
  unsigned long long* item_t0;   // [n_own]   wall clock (100 MHz) at which the item's owner started; 0: not yet
  uint32_t* help_head;           // [queries] (unused since round 6: the helpers' slots were a linked list per query)
  uint32_t* help_query;          // [n_help]  the query helper slot h worked for, + 1 (0: the slot was not used): what the merge reads
  uint32_t* help_off;            // [1]       a helper found nothing left worth joining: the later ones leave at once
  uint32_t* item_next;           // [1]       the next item of the launch order to be started
  uint32_t* help_used;           // [1]       helper slots handed out
  unsigned long long* t_start;   // [1]       wall clock at which item 0 started
  uint32_t n_own, n_help;        // items of the launch, workgroups launched beyond them
  uint32_t slot_base;            // output slot (item_keys / item_counts / item_hits) of helper 0
  uint32_t min_rem;              // bits 0-15: an item with fewer unassigned windows is not joined; bit 16: A/B, greedy choice
  uint32_t total_wins;           // windows of all items (the launch's progress = windows handed out / this)
  uint32_t alpha16;              // critical path: help while items are queued when an item's time left > alpha16 / 16 x the launch's; 0: never
  uint32_t n_cus;
  uint32_t persistent;           // 1: the launch has one workgroup per CU and each chooses work until none is left (maxscore.hip)
  unsigned long long* spec_g;    // [queries] the largest SPECULATIVE theta a workgroup has published for the query (kMsSpec*), 0 = none;
                                 // nullptr: no speculation in this launch
  uint32_t spec_z16, spec_sched; // the estimate's safety margin in standard deviations x 16; when estimates are due: bits 0-7 the
                                 // first one (doc windows begun by the workgroup), bits 8-15 the factor x 16 between one and the next
                                 // bit 16 (development build, A/B): the estimate is made in a meeting of all waves, not by one wave
                                 // bit 17 (development build, A/B): no half groups -- a window's last instruction runs the full body too
                                 // bit 18 (development build, A/B): an overflow compaction keeps the k best keys, dead ones included
  unsigned long long* walls;     // instrumented kernel only, else nullptr: per output slot 8 words -- {start, end} on the 100 MHz
                                 // wall clock, item, windows walked, when the workgroup's round began, CU id, round, workgroup --
                                 // when every piece of the launch ran, on one time base (nrtgpu_get_maxscore_item_walls)
};

// What one launch of bm25_maxscore_kernel works on: ONE record next to the plan, the kernel's only argument (maxscore.hip reads
// its fields where it uses them).
struct DExchange;
struct MsArgs {
  const DItem* items;            // [help.n_own] in launch order
  const DPart* parts;
  const DTerm* terms;
  const DQuery* queries;
  const float* caches;           // the queries' normInverse tables
  unsigned long long* theta_g;   // per query: the best theta any of its items (or their helpers) has published
  uint32_t* slice_sum;           // per (query, searcher slice): hits counted
  uint32_t* q_prune;             // per query: a slice has passed the floor (kMsModeCount)
  const DExchange* xch;          // cross-GPU bound exchange, or nullptr
  uint64_t* item_keys;           // per output slot k_stride keys ...
  uint32_t* item_counts;         // ... how many ...
  uint64_t* item_hits;           // ... and the hits counted there
  uint64_t* item_prof;           // instrumented kernel: 16 counters per output slot, else nullptr
  const uint32_t* q_wins;        // per query: the doc windows of all its items (speculation: the denominator of "how much have I seen")
  const DWalkRow* rows;          // the walk rows, indexed like `terms` (development build, A/B: nullptr = the walk works the bounds out itself)
  uint32_t k_stride;
  uint32_t scatter;              // != 0: an item's doc windows are handed out in a SCATTERED order (maxscore.hip): whatever a workgroup
                                 // has walked so far is spread over the item's docs like a sample -- what the speculative thresholds
                                 // assume -- also where the docid order follows time or a sort key
  DHelp help;
};

// Cross-GPU bound exchange of one batch (nrtgpu_exchange_open): entry (rank r, query q) of the batch's
// slot holds (tag << 32) | score word that at least ceil(k / world) docs of rank r's shard reach.
constexpr int kExchangeSlots = 8;
struct alignas(16) DExchange {
  unsigned long long* slot;  // this batch's [world][stride] entries (host-mapped, system scope)
  uint32_t world, rank;
  uint32_t stride;           // entries per rank (max_batch)
  uint32_t tag;              // epoch tag, != 0
};
static_assert(sizeof(DExchange) == 32, "DExchange layout");

// Packed hit: larger key == better hit under Lucene's HitQueue order (score desc, doc asc).
// Scores are >= 0 (BM25 weights are non-negative) so float bits order like the floats.
// One leaf's vector field as the hybrid tail sees it (doc -> row lookups happen on the device).
struct DVecSeg {
  const float* vecs;          // n_vec x dim fp32, row-major; nullptr: the leaf has no vectors for the field
  const float* vnorm2;        // |v|^2 per row
  const int32_t* ord_to_doc;  // ascending; nullptr: row == docid
  int32_t doc_base, max_doc, n_vec, pad;
};
static_assert(sizeof(DVecSeg) == 40, "DVecSeg layout");

// A leaf as the sketch kernel sees it (knn.hip: knn_sketch_kernel walks ALL leaves of a search in one launch: an NRT index is
// dozens of segments, and a launch per leaf cost 17 % of a pass at 40 leaves, 84 % at 160).  The leaves' tiles of 16 rows are
// numbered through: leaf i holds tiles [tile_begin, tile_begin + ceil(n_rows / 16)).
struct alignas(16) DKnnLeaf {
  const void* sketch;          // the leaf's fp16 sketch (tile 0 first)
  const float* vnorm2;         // |v|^2 per row (allocation padded by 64 B: a tile's 16 norms are read whole)
  const int32_t* ord_to_doc;   // nullptr: row == docid
  const uint64_t* accept;      // liveDocs (& filter) bits of the leaf; nullptr: every doc
  int64_t tile_begin;
  int32_t n_rows, doc_base;
  float inv_rows_scale;        // 1 / the power of two the rows were multiplied by
  int32_t pad;
  const uint64_t* const* accept_of;   // nullptr, or the leaf's row of the pass's accept table (kKnnAcceptCols below): `accept` per query
};
static_assert(sizeof(DKnnLeaf) == 64, "DKnnLeaf layout");
// A pass whose queries carry filters of their own (nrtgpu_knn_search_requests) brings a table of accept sets next to the leaves:
// kKnnAcceptCols pointers per leaf, entry q = liveDocs & query q's filter on that leaf (nullptr: every doc).  Columns at or beyond
// the pass's queries hold nullptr and are never read.  Without a table (nullptr) every query takes DKnnLeaf::accept.  The sketch
// kernel finds a leaf's row in its DKnnLeaf; the fp32 row kernel (a launch per leaf) is handed the row in place of the leaf's set,
// said by a bit of its `mode` argument.
constexpr int kKnnAcceptCols = 64;
constexpr int32_t kKnnAppendOnly = 1, kKnnAcceptTable = 2;   // knn_score_kernel's mode

// Exact vector search: the matrix-core ESTIMATE of a score against the RESULT (the same similarity summed in the oracle's
// order).  e_abs bounds |estimate - result| -- for EUCLIDEAN of the squared distance (the score 1 / (1 + d2) flattens with d2: a
// bound in score units would be useless for far rows), else of the score with the boost applied; e_rel covers the roundings of
// the map to a score.  DESIGN 4.5.
//   knn_result_upper: no row whose estimate is <= m has a result above this.
//   knn_estimate_lower: every row whose result is >= s has an estimate of at least this.
__host__ __device__ inline double knn_result_upper(int sim, double m, double e_abs, double e_rel, double boost) {
  if (sim == 2) {
    if (!(m > 0.0)) return 0.0;
    const double d2 = boost / m - 1.0;
    const double lo = d2 - (e_abs + e_rel * (1.0 + d2));
    return boost / (1.0 + (lo > 0.0 ? lo : 0.0)) * (1.0 + 1e-6);
  }
  return (m + e_abs + e_rel * (m < 0.0 ? -m : m)) * (1.0 + 1e-6);
}
__host__ __device__ inline double knn_estimate_lower(int sim, double s, double e_abs, double e_rel, double boost) {
  if (sim == 2) {
    if (!(s > 0.0)) return 0.0;
    const double d2 = boost / s - 1.0;
    return boost / (1.0 + (d2 > 0.0 ? d2 : 0.0) + e_abs + e_rel * (1.0 + d2)) * (1.0 - 1e-6);
  }
  return (s - (e_abs + e_rel * (s < 0.0 ? -s : s))) * (1.0 - 1e-6);
}

// Byte (int8) vector fields (knn_bytes.hip).  A leaf as knn_bytes_kernel sees it: the rows as tiles of 16 in the operand order of
// v_mfma_i32_16x16x64_i8 -- tile t, step s (64 dimensions), lane l: 16 bytes = row 16t + (l & 15), dimensions 64s + 16(l >> 4) .. +15;
// 1 KiB per (tile, step), a leaf's tiles contiguous -- and |v|^2 per row as int32.
struct alignas(16) DKnnBytesLeaf {
  const void* tiles;
  const int32_t* vnorm2;       // allocation padded to whole tiles: a tile's 16 norms are read whole
  const int32_t* ord_to_doc;   // nullptr: row == docid
  const uint64_t* accept;      // liveDocs (& filter) bits of the leaf; nullptr: every doc
  int64_t tile_begin;
  int32_t n_rows, doc_base;
  const uint64_t* const* accept_of;   // nullptr, or the leaf's row of the pass's accept table (kKnnAcceptCols above): `accept` per query --
                                      // read by knn_bytes_requests_kernel only, as DKnnLeaf::accept_of by the sketch kernel
  int32_t pad[2];
};
static_assert(sizeof(DKnnBytesLeaf) == 64, "DKnnBytesLeaf layout");
// One leaf's byte vector field as the rescorers see it (knn_bytes.hip: hybrid_rescore_bytes_kernel maps a hit's doc to its row on
// the device, as hybrid_rescore_kernel does through DVecSeg): the same tiles, the only copy of the rows.
struct DByteVecSeg {
  const void* tiles;          // nullptr: the leaf has no vectors for the field
  const int32_t* vnorm2;      // |v|^2 per row
  const int32_t* ord_to_doc;  // ascending; nullptr: row == docid
  int32_t doc_base, max_doc, n_vec, pad;
};
static_assert(sizeof(DByteVecSeg) == 40, "DByteVecSeg layout");

// The GATHER route of the filtered knn entries (knn.hip: knn_accept_rows_kernel, knn_gather_score_kernel; knn_bytes.hip:
// knn_gather_bytes_kernel): a leaf as those kernels see it.  The leaves' ordinals are numbered through: leaf i holds
// [row_begin, row_begin + n_rows).  An entry of the call's row list is (leaf << 32) | ordinal inside the leaf.
struct alignas(16) DKnnGatherLeaf {
  const void* rows;            // float field: n_rows x dim fp32, row-major; byte field: the tiles (DKnnBytesLeaf.tiles)
  const int32_t* vnorm2;       // byte field: |v|^2 per row; float field: unused (the oracle's order sums it with the dot product)
  const int32_t* ord_to_doc;   // nullptr: row == docid
  const uint64_t* accept;      // liveDocs & filter bits of the leaf (never nullptr on this route)
  int64_t row_begin;
  int32_t n_rows, doc_base;
  int32_t max_doc, pad[3];
};
static_assert(sizeof(DKnnGatherLeaf) == 64, "DKnnGatherLeaf layout");

// The UNBOOSTED score of one (query, row) pair of a byte vector field from its three integers dot = sum q_i v_i, nq = sum q_i^2,
// nv = sum v_i^2 -- ByteVectorFieldDef.similarityToScore's four shapes (VectorFieldDef.java:870-881) over what Lucene's
// VectorSimilarityFunction.compare(byte[], byte[]) hands it [Lucene-recall].  Every operation is one fp32 (cosine: fp64, then one
// cast) operation rounded once; int -> float conversions round to nearest even.  The ONE statement of it: knn_bytes_kernel and
// nrtgpu_byte_vector_score both call this function.  dim: the field's own dimension.  A zero vector under cosine scores 0.
__host__ __device__ inline float knn_byte_score(int sim, int32_t dim, int32_t dot, int32_t nq, int32_t nv) {
  if (sim == 0) {
    if (nq == 0 || nv == 0) return 0.0f;
    const float c = (float)((double)dot / sqrt((double)nq * (double)nv));
    return (1.0f + c) / 2.0f;
  }
  if (sim == 1) return 0.5f + (float)dot / (float)(dim * 32768);
  if (sim == 2) {
    const int32_t d2 = nq + nv - 2 * dot;   // == sum (q_i - v_i)^2: < 2^28 at dim <= 2048
    return 1.0f / (1.0f + (float)d2);
  }
  const float x = (float)dot;
  return x < 0.0f ? 1.0f / (1.0f + -1.0f * x) : x + 1.0f;
}

// What a launch of either final-score kernel (finalscore.hiph; finalscore.cpp) works on besides its route's own records: the
// exhaustive scan's plan records and item outputs.
struct FinalScoreArgs {
  uint32_t n_items;              // workgroups
  const DItem* items;
  const DPart* parts;
  const DTerm* terms;
  const DQuery* queries;
  const float* caches;           // the queries' normInverse tables
  unsigned long long* theta_g;   // per query: the best FINAL key bound any of its items has published
  uint32_t* slice_sum;           // per (query, searcher slice): hits counted
  uint32_t* slice_past;          // ... and, for the routes that count them (finalscore.cpp), those behind the query's cursor; else nullptr
  uint64_t* item_keys;           // per item k_stride keys ...
  uint32_t* item_counts;         // ... how many ...
  uint64_t* item_hits;           // ... and the hits counted there
  uint32_t k_stride;
  void* own;                     // the route's own zeroed workspace bytes (finalscore.cpp: FinalScoreOwn), nullptr: the route asked for none
  void* own_user;                // FinalScoreOwn.user: what the route's launcher and its collect() share on the host
};

// Function-score queries (funcscore.hip: bm25_function_score_kernel; funcscore.cpp): MultiFunctionScoreQuery over a BM25
// disjunction with weight functions only -- per doc a boost from the function sets it lies in.  One record per query of the call,
// and per part of the plan (same index as DPart) the resident doc set of every function on the part's leaf.
constexpr int kMaxFunctions = 8;
constexpr int kFsCandCap = 3072;    // the kernel's LDS candidate slots: >= kMaxK + kTileDocs (the k kept + one wave's whole sub-tile always fit)
static_assert(kFsCandCap >= kMaxK + kTileDocs, "function-score candidate buffer too small");
struct alignas(16) DFuncQuery {
  int32_t n_functions;              // 0..kMaxFunctions
  int32_t score_mode;               // 0 SCORE_MODE_MULTIPLY, 1 SCORE_MODE_SUM
  int32_t boost_mode;               // 0 BOOST_MODE_MULTIPLY, 1 BOOST_MODE_SUM, 2 BOOST_MODE_REPLACE
  int32_t min_excluded;
  float   min_score;
  uint32_t pad[3];
  float   weight[kMaxFunctions];    // FilterFunction.getWeight(), in the request's order
};
static_assert(sizeof(DFuncQuery) == 64, "DFuncQuery layout");
struct alignas(16) DFuncMasks {
  const uint64_t* mask[kMaxFunctions];   // liveDocs & the function's filter on the part's leaf; nullptr: every doc is in the set
};
static_assert(sizeof(DFuncMasks) == 64, "DFuncMasks layout");

// The score of one doc under a function-score query -- MultiFunctionScoreQuery.java:445-500 (MultiFunctionScorer.score,
// computeFunctionScore, computeFinalScore) with WeightFilterFunction.java:66-71 -- and whether the doc is a hit (the minScore
// wrapper, :60-65 and :334-336).  matched: bit i = the doc lies in function i's set.  inner: the inner query's float score.
// Every operation is one IEEE operation rounded once.  The ONE statement of it: bm25_function_score_kernel and
// nrtgpu_function_score_value both call this function (f is read where it lies: no indexed copy in registers).
__host__ __device__ inline float function_score_value(const DFuncQuery& f, uint32_t matched, float inner, bool* is_hit) {
  float final_score = inner;
  if (f.n_functions != 0) {
    double fs;
    if (f.score_mode == 0) {
      fs = 1.0;
      for (int i = 0; i < f.n_functions; ++i)
        if ((matched >> i) & 1u) fs *= (double)f.weight[i];
    } else {
      fs = 0.0;
      bool any = false;
      for (int i = 0; i < f.n_functions; ++i)
        if ((matched >> i) & 1u) {
          fs += (double)f.weight[i];
          any = true;
        }
      if (!any) fs = 1.0;
    }
    final_score = f.boost_mode == 0 ? (float)((double)inner * fs) : (f.boost_mode == 1 ? (float)((double)inner + fs) : (float)fs);
  }
  *is_hit = true;
  if (f.min_score > 0.0f || f.min_excluded != 0)
    *is_hit = final_score > f.min_score || (f.min_excluded == 0 && final_score == f.min_score);
  return final_score;
}

// A text query beside knn clauses (knnclauses.hip: bm25_text_knn_kernel; knnclauses.cpp): the request's `query` and its resolved
// `knn` lists as SHOULD clauses of one BooleanQuery.  Beside the plan go the listed docs per (query, leaf) -- sorted leaf-local
// docids and their knn_sum doubles, duplicates across lists merged, structure of arrays -- and one record per part of the plan
// (same index as DPart).
struct alignas(16) DKnnPart {
  const uint64_t* live_bits;   // the LEAF's own liveDocs words (nullptr: all live): DPart.live_bits is the query's accept set, and
                               // nullptr there when liveDocs are folded into the postings
  uint32_t entry_begin, entry_end;   // the (query, leaf)'s entries inside the part's tile range
  uint32_t nested;             // the query's form: 0 FLAT, 1 NESTED
  uint32_t pad[3];
};
static_assert(sizeof(DKnnPart) == 32, "DKnnPart layout");
// A slot the tag pass has finished: bit 63, and the doc's final float in the low 32 bits.  An untagged slot holds a fixed-point
// sum: at most kMaxTerms clauses of values below 2^32 shifted left by at most 15 bits (planner.cpp: resolve_queries) -- below
// 2^52, so bit 63 is never a sum's.
constexpr uint64_t kKnnTag = 1ull << 63;
static_assert(kMaxTerms <= 32, "a fixed-point sum must stay below 2^52 (32 clauses x 2^32 x 2^15): bit 63 is the tag");
// The score of one doc under text + knn clauses [Lucene-recall].  text_matched: the doc matches the text query AND lies in its
// accept set; fixed_sum: the double sum of its text clauses as the accumulators hold it (x 2^fx_E, exact); knn_sum: the double
// sum, in list order, of the values of the lists that hold the doc, 0 when none does (a value is > 0).  Every operation is one
// IEEE operation rounded once.  The ONE statement of it: bm25_text_knn_kernel and nrtgpu_text_knn_value both call this function.
//   BooleanQuery.rewrite inlines a pure SHOULD disjunction into the outer query (FLAT: one double sum over all clauses, one
//   cast); any other text query stays ONE clause whose float score is added (NESTED).
__host__ __device__ inline float text_knn_value(uint32_t nested, bool text_matched, uint64_t fixed_sum, int fx_E, double knn_sum) {
  const double text = text_matched ? ldexp((double)fixed_sum, -fx_E) : 0.0;   // fixed_sum < 2^53: exact conversion, exact scaling
  if (!text_matched) return (float)knn_sum;
  if (knn_sum == 0.0) return (float)text;   // the text query alone: what nrtgpu_search_bm25 scores
  return nested != 0u ? (float)((double)(float)text + knn_sum) : (float)(text + knn_sum);
}

// Multi-match queries (multimatch.hip: bm25_multi_match_kernel; multimatch.cpp): two-level queries over term clauses -- a
// BooleanQuery over DisjunctionMaxQuery groups (cross_fields) or a DisjunctionMaxQuery over BooleanQuery groups (best_fields).
// The plan is the exhaustive route's over the clauses as one SHOULD disjunction; beside it one DGroupQuery per query, and every
// clause's group in its DQTerm.tab_slot (copied verbatim to the DTerms: bits no scorer reads).
constexpr int kMaxGroups = 8;
constexpr uint32_t kTabSlotGroupShift = 24, kTabSlotGroupMask = 31u;   // DTerm.tab_slot bits 24-28: the clause's group (this route only)
constexpr uint32_t kGroupsSumOfMax = 0, kGroupsMaxOfSum = 1;           // DGroupQuery.shape (nrtgpu.h: NRTGPU_GROUPS_*)
// The kernel's workgroup: per wave a sub-tile's u64 sums (8 KiB) AND u32 maxima (4 KiB) -- 12 waves of that leave no room for
// the candidate buffer in 160 KiB, so 8 waves (two per SIMD: 256 VGPRs each, which hold the docs' outer state).
constexpr int kMmWaves = 8;
constexpr int kMmThreads = kMmWaves * 64;
constexpr int kMmCandCap = 2048;    // == kMaxK + kTileDocs: the k kept + one wave's whole sub-tile always fit; <= 4 x kMmThreads (topk.hiph)
static_assert(kMmCandCap >= kMaxK + kTileDocs && kMmCandCap <= 4 * kMmThreads, "multi-match candidate buffer");
struct alignas(16) DGroupQuery {
  uint32_t shape;                   // kGroups*
  uint32_t n_groups;                // 1..kMaxGroups
  float    tie_breaker;             // of the DisjunctionMax level
  uint32_t group_occur;             // kGroupsSumOfMax: 0 the groups are SHOULD clauses, 1 MUST
  uint32_t min_should_match;        // kGroupsSumOfMax, SHOULD groups: the query's minimumNumberShouldMatch
  uint32_t pad[3];
  uint8_t  occur[kMaxGroups];       // kGroupsMaxOfSum: 1 = the group's clauses are MUST
  uint8_t  min_match[kMaxGroups];   // kGroupsMaxOfSum, SHOULD group: its minimumNumberShouldMatch (saturated at 255: more than any group holds)
  uint8_t  n_clauses[kMaxGroups];   // the group's clauses in the QUERY (also those whose term no leaf holds)
  uint8_t  pad2[kMaxGroups];
};
static_assert(sizeof(DGroupQuery) == 64, "DGroupQuery layout");

// DisjunctionMaxScorer's score from the best sub-score and the double sum of ALL sub-scores: (float)(scoreMax + otherScoreSum *
// tieBreaker) with otherScoreSum = sum - max.  The statement the flat DisjunctionMax route makes on its fixed-point pair
// (maxscore.hip: kMsSecTieBreaker); here both levels of a multi-match query call it.
__host__ __device__ inline float disjunction_max_value(float best, double sum, float tie_breaker) {
  return (float)((double)best + (sum - (double)best) * (double)tie_breaker);
}
// What a doc has collected over the groups handled so far: folded group by group, in group order.
struct MmOuter {
  double sum;      // of the matching groups' scores
  float  best;     // the largest of them
  uint32_t n;      // matching groups
};
// The score of group g for a doc from the group's double sum, best clause score and number of matching clauses (> 0), and
// whether the group matches the doc at all.  Every operation is one IEEE operation rounded once.
__host__ __device__ inline bool multi_match_group(const DGroupQuery& r, uint32_t g, double sum, float best, uint32_t count, float* score) {
  if (r.shape == kGroupsSumOfMax) {
    *score = disjunction_max_value(best, sum, r.tie_breaker);
    return count != 0u;
  }
  const uint32_t need = r.occur[g] != 0 ? (uint32_t)r.n_clauses[g] : (r.min_match[g] > 1 ? (uint32_t)r.min_match[g] : 1u);
  *score = (float)sum;
  return count >= need;
}
__host__ __device__ inline void multi_match_fold(MmOuter& o, float group_score) {
  o.sum += (double)group_score;
  o.best = group_score > o.best ? group_score : o.best;
  o.n += 1u;
}
// The doc's final score from its outer state, and whether it is a hit.  The ONE statement of it: bm25_multi_match_kernel and
// nrtgpu_multi_match_value both call these three functions.
__host__ __device__ inline float multi_match_value(const DGroupQuery& r, const MmOuter& o, bool* is_hit) {
  if (r.shape == kGroupsSumOfMax) {
    *is_hit = r.group_occur != 0 ? o.n == r.n_groups : o.n >= (r.min_should_match > 1u ? r.min_should_match : 1u);
    return (float)o.sum;
  }
  *is_hit = o.n != 0u;
  return disjunction_max_value(o.best, o.sum, r.tie_breaker);
}

__host__ __device__ inline uint64_t pack_key(float score, uint32_t global_doc) {
  union { float f; uint32_t u; } c;
  c.f = score;
  return ((uint64_t)c.u << 32) | (uint64_t)(0xFFFFFFFFu - global_doc);
}
__host__ __device__ inline float key_score(uint64_t key) {
  union { float f; uint32_t u; } c;
  c.u = (uint32_t)(key >> 32);
  return c.f;
}
__host__ __device__ inline uint32_t key_doc(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// Sort by field (fieldsort.hip: bm25_field_sort_kernel; fieldsort.cpp): a text query's hits ordered by a per-doc value column of
// the segment store (segment.cpp: nrtgpu_segment_add_doc_values) instead of by score.  The column is resident as the ascending
// ORDER-PRESERVING CODE of the values: unsigned compares of codes order like Integer.compare / Float.compare of the values.
//   kDocValuesInt32   : bits ^ 0x80000000
//   kDocValuesFloat32 : NaNs canonicalised to 0x7FC00000, then negative floats ~bits, the others bits | 0x80000000:
//                       -0.0 < +0.0, NaN above +inf (Float.compare)
// The key of a hit is (sort_key_high << 32) | (0xFFFFFFFF - doc): the k LARGEST keys are the page, so an ascending sort
// complements the code; equal values rank by docid ascending in both directions.  A key is never 0 (docids stay below 2^31).
// The ONE statement of the coding: the upload, bm25_field_sort_kernel, the host's decode of the hits and
// nrtgpu_sort_value_code all call these functions.
constexpr int kDocValuesInt32 = 0, kDocValuesFloat32 = 1;
__host__ __device__ inline uint32_t doc_value_code(int kind, uint32_t bits) {
  if (kind == kDocValuesInt32) return bits ^ 0x80000000u;
  if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = 0x7FC00000u;
  return (bits & 0x80000000u) != 0u ? ~bits : bits | 0x80000000u;
}
__host__ __device__ inline uint32_t doc_value_bits(int kind, uint32_t code) {   // the inverse (a NaN comes back canonical)
  if (kind == kDocValuesInt32) return code ^ 0x80000000u;
  return (code & 0x80000000u) != 0u ? code & 0x7FFFFFFFu : ~code;
}
__host__ __device__ inline uint32_t sort_key_high(uint32_t reverse, uint32_t code) { return reverse != 0u ? code : ~code; }
__host__ __device__ inline uint64_t sort_key(uint32_t reverse, uint32_t code, uint32_t global_doc) {
  return ((uint64_t)sort_key_high(reverse, code) << 32) | (uint64_t)(0xFFFFFFFFu - global_doc);
}
// One record per query of the call, and per part of the plan (same index as DPart) the column on the part's leaf.
struct alignas(16) DSortQuery {
  uint32_t reverse;        // SortField.getReverse()
  uint32_t missing_code;   // what a doc without a value sorts as
  uint32_t need;           // clauses a hit matches at least: max(1, minimumNumberShouldMatch), or all of them (MUST)
  uint32_t has_after;
  uint64_t after_key;      // searchAfter: only keys below it are collected (hits of earlier pages still count)
  uint32_t pad[2];
};
static_assert(sizeof(DSortQuery) == 32, "DSortQuery layout");
struct alignas(16) DSortPart {
  const uint32_t* code;    // one code per doc, padded to whole sub-tiles; nullptr: the leaf lacks the column
  const uint64_t* has;     // bit d: doc d has a value; nullptr: every doc has
                           // A MULTI-VALUED column (below: kTermsQueryMulti / DRangeQuery.multi say which are; the kernels of such calls
                           // alone read one): `code` is codes[], the values' codes in upload order, and `has` is the uint32 start[]
                           // -- one entry per doc, padded to whole sub-tiles, plus one; doc d's values are codes[start[d] ..
                           // start[d + 1]); every padding entry equals the number of values
};
static_assert(sizeof(DSortPart) == 16, "DSortPart layout");

// Sort by a 64-BIT column (fieldsort64.hip: bm25_field_sort64_kernel; docset.hip: docset_sort_kernel under DocsetSort64; fieldsort64.cpp): LONG /
// DATE_TIME (epoch millis) / DOUBLE doc values.  The column is resident as 64-bit order-preserving codes -- unsigned compares of
// codes order like Long.compare / Double.compare of the values:
//   kDocValuesInt64   : bits ^ 1 << 63
//   kDocValuesFloat64 : NaNs canonicalised to 0x7FF8000000000000, then negative doubles ~bits, the others bits | 1 << 63:
//                       -0.0 < +0.0, NaN above +inf (Double.compare)
// The top-k's keys stay 64 bits: a call's global docids need db bits (the leaves' bases and sizes say how many), the codes of
// the sort's column over the call's leaves lie in [lo, lo + span] (recorded at upload), and a key packs a value's ORDINAL in that
// window above a db-bit docid field -- lossless whenever the ordinals fit the 64 - db bits the docids leave (sort64_fits; a sort
// that does not fit is refused, not widened).  Ascending ordinal u of a code c: 0 below lo, 1 + (c - lo) inside, span + 2 above
// hi.  Only the sort's MISSING value can lie outside the window (its code stands for the docs without a value), so the two
// sentinels lose nothing.  The key's value field is f = reverse ? u + 1 : (span + 2 - u) + 1, in [1, span + 3]; key =
// (f << db) | ((1 << db) - 1 - global_doc): the k LARGEST keys are the page, equal values rank by docid ascending in both
// directions, a key is never 0.  The searchAfter cursor is tested on (code, doc), NOT on keys: a cursor value outside the window
// that is not the missing value would collapse onto a sentinel (sort64_behind).
// The ONE statement of all of it: the upload, both kernels, the host's decode of the hits, nrtgpu_sort_key64 and
// nrtgpu_range_accepts64 call these functions.
constexpr int kDocValuesInt64 = 2, kDocValuesFloat64 = 3;
__host__ __device__ inline uint64_t doc_value_code64(int kind, uint64_t bits) {
  if (kind == kDocValuesInt64) return bits ^ 0x8000000000000000ull;
  if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) bits = 0x7FF8000000000000ull;
  return (bits & 0x8000000000000000ull) != 0ull ? ~bits : bits | 0x8000000000000000ull;
}
__host__ __device__ inline uint64_t doc_value_bits64(int kind, uint64_t code) {   // the inverse (a NaN comes back canonical)
  if (kind == kDocValuesInt64) return code ^ 0x8000000000000000ull;
  return (code & 0x8000000000000000ull) != 0ull ? code & 0x7FFFFFFFFFFFFFFFull : ~code;
}
__host__ __device__ inline bool range_accepts_code64(uint64_t lo_code, uint64_t hi_code, uint64_t code) { return code >= lo_code && code <= hi_code; }
// span + 3 <= 2^(64 - db) - 1, without overflow (span may be 2^64 - 1); db in 1..31
__host__ __device__ inline bool sort64_fits(uint64_t span, uint32_t db) { return span <= (1ull << (64u - db)) - 4ull; }
// the bits the value field of a window needs: bit_length(span + 3), 65 where that overflows (for the refusal's reason)
__host__ inline int sort64_value_bits(uint64_t span) {
  if (span > ~0ull - 3ull) return 65;
  int b = 0;
  for (uint64_t f = span + 3ull; f != 0ull; f >>= 1) ++b;
  return b;
}
__host__ __device__ inline uint64_t sort64_ordinal(uint64_t lo, uint64_t span, uint64_t code) {
  if (code < lo) return 0ull;
  const uint64_t off = code - lo;
  return off <= span ? 1ull + off : span + 2ull;
}
__host__ __device__ inline uint64_t sort_key64(uint32_t reverse, uint64_t lo, uint64_t span, uint32_t db, uint64_t code, uint32_t global_doc) {
  const uint64_t u = sort64_ordinal(lo, span, code);
  const uint64_t f = (reverse != 0u ? u : span + 2ull - u) + 1ull;
  return (f << db) | (uint64_t)(((1u << db) - 1u) - global_doc);
}
// whether (code, doc) ranks strictly behind the cursor (after_code, after_doc) in the sort's order
__host__ __device__ inline bool sort64_behind(uint32_t reverse, uint64_t code, uint32_t global_doc, uint64_t after_code, uint32_t after_doc) {
  if (code != after_code) return (reverse != 0u) == (code < after_code);
  return global_doc > after_doc;
}
// the host's decode of a returned key: the doc, and the ascending ordinal of the value it sorted as
__host__ inline void sort_key64_decode(uint32_t reverse, uint64_t span, uint32_t db, uint64_t key, uint32_t* global_doc, uint64_t* ordinal) {
  const uint64_t f = (key >> db) - 1ull;
  *global_doc = ((1u << db) - 1u) - (uint32_t)(key & (uint64_t)((1u << db) - 1u));
  *ordinal = reverse != 0u ? f : span + 2ull - f;
}
// One record per query of the call, and per part of the plan (same index as DPart) the 64-bit column on the part's leaf.
struct alignas(16) DSort64Query {
  uint64_t lo, span;       // the window of the column's codes over the call's leaves
  uint64_t missing_code;   // what a doc without a value sorts as
  uint64_t after_code;     // searchAfter: the cursor's code ...
  uint32_t after_doc;      // ... and global docid; only docs behind it are collected (hits of earlier pages still count)
  uint32_t has_after;
  uint32_t reverse;        // SortField.getReverse()
  uint32_t need;           // DSortQuery.need
  uint32_t db;             // bits of the key's docid field
  uint32_t pad[3];
};
static_assert(sizeof(DSort64Query) == 64, "DSort64Query layout");
struct alignas(16) DSort64Part {
  const uint64_t* code64;  // one 64-bit code per doc, padded to whole sub-tiles; nullptr: the leaf lacks the column
  const uint64_t* has;     // bit d: doc d has a value; nullptr: every doc has
};
static_assert(sizeof(DSort64Part) == 16, "DSort64Part layout");
static_assert(sizeof(DSort64Part) == sizeof(DSortPart), "a per-part column record is read as either (the range facets' count column; docset.cpp's part walk)");

// Terms aggregation (termscount.hip: bm25_terms_count_kernel, terms_compact_kernel; termscount.cpp): a query's hits counted per
// distinct value of a doc value column.  A bucket is a column CODE (doc_value_code: ints by value, floats by floatToIntBits with
// every NaN in one bucket).  Count tables are open-addressed, a slot one 64-bit word (count << 32) | code, 0 = empty (a slot
// that is in use counts at least 1): a workgroup's table in LDS as a combiner, the query's table in global memory, which the
// query's items share.  The home slot of a code is the top bits of code * kTermsHashMul (codes that agree in their low bits
// spread); probing is linear and BOUNDED: kTermsLdsProbe steps in LDS (then the value goes straight to the global table), the
// table's capacity in global memory (then the query's overflow flag is raised).  Every slot claimed in a query's global table
// counts in DTermsState.claimed: a query overflows iff its hits hold more than max_buckets distinct values, whatever the load.
constexpr int kTermsLdsSlots = 8192;          // 64 KiB of the workgroup's LDS
constexpr int kTermsLdsShift = 32 - 13;       // home slot = hash >> shift
constexpr int kTermsLdsProbe = 8;
static_assert((1 << (32 - kTermsLdsShift)) == kTermsLdsSlots, "the LDS table's hash shift");
constexpr uint32_t kTermsHashMul = 0x9E3779B1u;
constexpr int kTermsMaxBuckets = 65536;                 // NRTGPU_MAX_TERM_BUCKETS
constexpr uint64_t kTermsMaxCallSlots = 1ull << 25;     // global table slots of one call, summed over its queries (256 MiB)
__host__ __device__ inline uint32_t terms_home_slot(uint32_t code, uint32_t shift) { return (code * kTermsHashMul) >> shift; }
// the slots of a query's global table: the power of two >= 2 x max_buckets (at least 2), as 32 - log2
__host__ inline uint32_t terms_table_shift(uint32_t max_buckets) {
  uint32_t log2 = 1;
  while ((1u << log2) < 2u * max_buckets) ++log2;
  return 32u - log2;
}
constexpr uint32_t kTermsQueryMulti = 1u << 31;   // DTermsQuery.need: the count column is multi-valued
static_assert((uint32_t)kMaxTerms < kTermsQueryMulti, "a clause count leaves DTermsQuery.need's top bit free");
struct alignas(16) DTermsQuery {
  uint32_t need;          // clauses a hit matches at least (DSortQuery.need); bit 31 (kTermsQueryMulti): the count column is
                          // multi-valued -- set in calls that launch the *_multi kernels only, which mask it off; a call whose
                          // named columns are all single-valued sets it nowhere, and its kernels read the word whole
  uint32_t max_buckets;
  uint32_t table_off;     // the query's global table: first slot ...
  uint32_t table_shift;   // ... and 32 - log2 of its slots
};
static_assert(sizeof(DTermsQuery) == 16, "DTermsQuery layout");
struct alignas(16) DTermsState {   // per query, zeroed per call; one more behind the last query: `claimed` = compacted entries of the call
  uint32_t claimed;       // slots claimed in the global table == distinct values seen (until the query overflows)
  uint32_t overflow;      // 1: more than max_buckets distinct values; the query's items stop counting values
  uint32_t n_out;         // terms_compact_kernel: the query's buckets ...
  uint32_t out_base;      // ... and where they begin among the call's compacted entries
};
static_assert(sizeof(DTermsState) == 16, "DTermsState layout");

// The terms aggregation over a 64-BIT column (termscount64.hip: bm25_terms_count64_kernel, terms_compact64_kernel; docset.hip:
// docset_terms_count64_kernel; termscount64.cpp): a bucket is a 64-bit column code (doc_value_code64: longs by value, doubles by
// doubleToLongBits with every NaN in one bucket).  A code does not fit beside its count in one word, so a slot is TWO words in
// two arrays: an 8-byte key and a 4-byte count.  Key 0 is "empty"; a key slot is claimed with ONE compare-and-swap (0 -> code)
// and never changes again, the count beside it grows by atomic adds only and is read behind the kernel (the compaction) or behind
// the workgroup's barrier (the flush) -- no thread ever waits for a slot to become complete.  EVERY 64-bit code is a value (code 0
// is Long.MIN_VALUE, code 2^64 - 1 Long.MAX_VALUE), so the one value whose code is the empty marker is counted BESIDE the table:
// a 4-byte counter of the workgroup in LDS, one of the query in its state record; the add that finds the query's counter at 0 is
// the value's first arrival and claims a bucket like any other.  Everything else is the 32-bit tables' contract, word for word:
// linear probing, kTermsLdsProbe steps in LDS (then the value goes straight to the query's table), the table's capacity in global
// memory (then the overflow flag); every claimed bucket counts in `claimed`; a query overflows iff its hits hold more than
// max_buckets distinct values, whatever the load (a query's table has the power of two >= 2 x max_buckets slots: it cannot fill
// before `claimed` passes the bound).  DTermsQuery is reused as it is (table_off: the query's first slot in both arrays).
// The home slot mixes BOTH halves of the code, each through a multiplier of its own: ids that differ only above bit 32 spread,
// and so do timestamps that differ only below it.  The ONE statement of it: the kernels and nrtgpu_terms_home_slots64 call
// terms_home_slot64.
constexpr int kTerms64LdsSlots = 8192;        // 96 KiB of the workgroup's LDS: 64 KiB of keys, 32 KiB of counts (NRTGPU_TERMS64_LDS_SLOTS)
constexpr int kTerms64LdsShift = 32 - 13;     // home slot = hash >> shift
static_assert((1 << (32 - kTerms64LdsShift)) == kTerms64LdsSlots, "the 64-bit LDS table's hash shift");
constexpr uint32_t kTerms64HashMulHigh = 0xC2B2AE3Du;   // the code's high word (the low word: kTermsHashMul)
constexpr uint64_t kTerms64SlotBytes = 12;              // a key and a count
constexpr uint64_t kTerms64MaxCallSlots = (1ull << 28) / kTerms64SlotBytes;   // 22 369 621: the 32-bit entry's 256 MiB of tables per call
__host__ __device__ inline uint32_t terms_home_slot64(uint64_t code, uint32_t shift) {
  return ((uint32_t)code * kTermsHashMul + (uint32_t)(code >> 32) * kTerms64HashMulHigh) >> shift;
}
struct alignas(16) DTermsState64 {   // DTermsState with the reserved code's counter; one more behind the last query, as there
  uint32_t claimed;       // buckets claimed (the reserved code's included) == distinct values seen (until the query overflows)
  uint32_t overflow;
  uint32_t n_out;
  uint32_t out_base;
  uint32_t zero_count;    // hits under code 0, the key that marks an empty slot
  uint32_t pad[3];
};
static_assert(sizeof(DTermsState64) == 32, "DTermsState64 layout");

// Doc-set requests (docset.hip: docset_sort_kernel, docset_count_kernel; docset.cpp): a sorted search or a terms count
// whose hit set is a doc set -- liveDocs, FILTER / MUST_NOT masks, numeric range clauses -- and no text clause.  The parts of
// such a plan have no clauses (n_terms == 0) and DPart.live_bits is the query's combined accept set WITH liveDocs (there are no
// postings to fold them into; nullptr: every doc below max_doc).  Beside the plan go the sorted / counting route's own records
// (DSortQuery / DTermsQuery per query, `need` unread; one DSortPart per part for the sort / count column), one DRangeQuery per
// query and kMaxRanges DSortPart per part (entry part * kMaxRanges + clause: the clause's column on the part's leaf).
// A range clause keeps a doc iff the doc HAS a value in the clause's column and code(lower) <= code(value) <= code(upper)
// (doc_value_code: unsigned compares of codes are Integer.compare / Float.compare of the values).  code(lower) > code(upper)
// keeps nothing.  The ONE statement of it: both kernels and nrtgpu_range_accepts call range_accepts_code.
constexpr int kMaxRanges = 4;   // NRTGPU_MAX_RANGES
__host__ __device__ inline bool range_accepts_code(uint32_t lo_code, uint32_t hi_code, uint32_t code) { return code >= lo_code && code <= hi_code; }
struct alignas(16) DRangeQuery {
  uint32_t n_ranges;            // 0..kMaxRanges
  uint32_t multi;               // bit r: clause r's column is multi-valued -- the doc passes iff SOME value of it is in the range
                                // (read under docset.hip's MULTI only: a call that sets a bit launches those kernels)
  uint32_t pad[2];
  uint32_t lo_code[kMaxRanges];
  uint32_t hi_code[kMaxRanges];
};
static_assert(sizeof(DRangeQuery) == 48, "DRangeQuery layout");

// Filter masks built from doc value columns (valuemask.hip: value_mask_kernel; valuemask.cpp:
// nrtgpu_segment_set_mask_from_values): the docs of ONE leaf that pass every clause of a call, as 64-bit words.  A clause tests the
// codes of one column of the leaf: a doc passes iff it HAS a value whose code passes; over a multi-valued column iff SOME value
// of it does.  The three clause kinds of the ABI are two tests here:
//   range    range_accepts_code(lo_code, hi_code, code) -- NRTGPU_CLAUSE_RANGE; NRTGPU_CLAUSE_EXISTS is the range of every code
//   in set   the code is one of set_len > 0 codes, sorted ascending without duplicates, at sets[set_off ...] of the call's code
//            array (NRTGPU_CLAUSE_IN_SET; lo_code / hi_code are the set's first and last code: one compare drops most values
//            before the search).  The ONE statement of the search: value_set_has, over the workgroup's LDS copy in the kernel.
constexpr int kMaxSetValues = 4096;      // NRTGPU_MAX_SET_VALUES: kMaxRanges sets fill the 64 KiB a launch may ask for
constexpr int kValueMaskThreads = 256;   // 4 waves; a wave owns whole 64-doc words
struct alignas(16) DValueClause {
  const uint32_t* code;    // DSortPart.code of the column; nullptr: the column holds no value, no doc passes
  const void* has;         // DSortPart.has: the uint64 `has` words (nullptr: every doc has) / multi != 0: the uint32 start[]
  uint32_t lo_code, hi_code;
  uint32_t set_off, set_len;   // set_len == 0: a range test
  uint32_t multi;          // the column is multi-valued
  uint32_t pad[3];
};
static_assert(sizeof(DValueClause) == 48, "DValueClause layout");
// The same over 64-BIT columns (valuemask.hip: value_mask64_kernel; nrtgpu_segment_set_mask_from_values64): range and exists
// clauses only, single-valued columns only; range_accepts_code64 over the column's 64-bit codes.
struct alignas(16) DValueClause64 {
  const uint64_t* code64;  // DSort64Part.code64 of the column; nullptr: no doc passes
  const uint64_t* has;     // DSort64Part.has (nullptr: every doc has)
  uint64_t lo_code, hi_code;
};
static_assert(sizeof(DValueClause64) == 32, "DValueClause64 layout");
// whether the sorted, duplicate-free set[0 .. len), len >= 1, holds code: a lower-bound search whose step count depends on len
// alone (the lanes of a wave stay together); every index read lies below len
template <class P>
__host__ __device__ inline bool value_set_has(P set, uint32_t len, uint32_t code) {
  uint32_t base = 0, n = len;
  while (n > 1u) {   // if the code is in the set, its index lies in [base, base + n)
    const uint32_t half = n >> 1;
    if (set[base + half] <= code) base += half;
    n -= half;
  }
  return set[base] == code;
}

// Numeric range facets (rangecount.hip: bm25_range_count_kernel; docset.hip: DocsetRanges; rangecount.cpp): a
// query's hits counted per requested value range [lower, upper], both inclusive, of a single-valued column of any of the four
// kinds.  Ranges may overlap, nest, repeat or touch, so the device does not count per range: it counts per ELEMENTARY INTERVAL
// (Lucene's LongRangeCounter construction [Lucene-recall]).  In code space (doc_value_code / doc_value_code64) the cut points of
// a query are every non-empty range's lo, and hi + 1 unless hi is the kind's greatest code (range_greatest_code: nothing lies
// above it), sorted without duplicates: n_cuts <= kMaxRangeCuts.  The interval of a code c is the number of cuts <= c, in
// 0..n_cuts; a range covers exactly the intervals interval(lo) .. interval(hi), and the host sums their counters.  The per-hit
// work -- one search, one 4-byte add -- does not depend on how the ranges lie.
// The ONE statement of the search and of the cut list: both kernels, the host's roll-up, nrtgpu_range_cuts and
// nrtgpu_range_interval call range_interval / range_cuts.
constexpr int kMaxCountRanges = 64;                    // NRTGPU_MAX_COUNT_RANGES
constexpr int kMaxRangeCuts = 2 * kMaxCountRanges;
// the number of cuts <= code among the ascending, duplicate-free cuts[0 .. n_cuts): a search whose step count depends on n_cuts
// alone; every index read lies below n_cuts.  A BOUND ends it, not a sentinel: a real code
// may equal the greatest code, so padding the list with it would miscount.
template <class P, class T>
__host__ __device__ inline uint32_t range_interval(P cuts, uint32_t n_cuts, T code) {
  uint32_t base = 0, n = n_cuts;   // cuts[0 .. base) are all <= code; the answer lies in [base, base + n]; base + n <= n_cuts
  while (n > 0u) {
    const uint32_t half = (n + 1u) >> 1;
    if (cuts[base + half - 1u] <= code) base += half;
    n -= half;
  }
  return base;
}
// the greatest code a value of the kind can have: INT_MAX / LONG_MAX for ints, the canonical NaN for floats
__host__ __device__ inline uint64_t range_greatest_code(int kind) {
  if (kind == kDocValuesInt32) return 0xFFFFFFFFull;
  if (kind == kDocValuesFloat32) return 0xFFC00000ull;
  if (kind == kDocValuesInt64) return 0xFFFFFFFFFFFFFFFFull;
  return 0xFFF8000000000000ull;
}
// the cut list of n_ranges ranges given as codes (lo[i] > hi[i]: an empty range, no cut): out[0 .. return), ascending without
// duplicates; out holds 2 x n_ranges entries
template <class T>
__host__ inline uint32_t range_cuts(const T* lo, const T* hi, uint32_t n_ranges, T greatest, T* out) {
  uint32_t n = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    if (lo[i] > hi[i]) continue;
    out[n++] = lo[i];
    if (hi[i] < greatest) out[n++] = (T)(hi[i] + 1);
  }
  for (uint32_t i = 1; i < n; ++i) {   // (insertion sort: at most 128 entries)
    const T v = out[i];
    uint32_t j = i;
    for (; j > 0 && out[j - 1] > v; --j) out[j] = out[j - 1];
    out[j] = v;
  }
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (m == 0 || out[m - 1] != out[i]) out[m++] = out[i];
  return m;
}
struct alignas(16) DRangeCountQuery {
  uint32_t need;          // clauses a hit matches at least (DSortQuery.need; unread by the doc-set kernel)
  uint32_t n_cuts;        // 0..kMaxRangeCuts
  uint32_t cut_off;       // the query's cuts in the call's cut array (uint32 codes, or uint64 for a call over 64-bit columns)
  uint32_t counter_off;   // the query's n_cuts + 1 interval counters among the call's uint32 counters
};
static_assert(sizeof(DRangeCountQuery) == 16, "DRangeCountQuery layout");

}  // namespace nrtgpu
