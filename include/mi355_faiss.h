/*
 * include/mi355_faiss.h -- C ABI of libmi355faiss.so, the MI355X-native replacement for the FAISS
 * calls the reference DuckDB extension makes on its vector-search hot path.
 *
 * Every entry point replaces ONE FAISS C++ symbol that /root/reference/src/faiss_extension.cpp (or
 * src/gpu/gpu.cpp) reaches; the citation after each declaration is that call site.  Plain pointers
 * and sizes only: the faiss::-namespaced C++ adaptor (duckdb-faiss-ext_amd/compat/faiss/...) and the
 * Python ctypes host (duckdb-faiss-ext_amd/pyhost/mi355_faiss.py) are both thin layers over this file,
 * and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - return 0 on success; nonzero = failure, text in mvs_last_error() (thread-local).  The text
 *     carries FAISS's exception message because the reference pattern-matches substrings of it:
 *       "should be at least as large as number of clusters"      src/faiss_extension.cpp:400,592
 *       "add_with_ids not implemented for this type of index"    src/faiss_extension.cpp:523
 *       "This index type is not implemented"                     src/gpu/gpu.cpp:52
 *       "Invalid GPU device"                                     src/gpu/gpu.cpp:56
 *   - x / ids / D / I are HOST pointers owned by the caller and valid only for the duration of the
 *     call (DuckDB vector buffers, new[] arrays: src/faiss_extension.cpp:626-627); the library
 *     copies through pinned staging.  The *_device variants take device pointers instead.
 *   - an index may be called from a different OS thread each time (DuckDB workers); calls on one
 *     index are serialised internally as the reference's faiss_lock does (:394,:506,:581,:629).
 *   - the product path has NO CPU fallback: every call fails loudly if no gfx950 device is usable.
 */
#ifndef MI355_FAISS_H
#define MI355_FAISS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* faiss::MetricType enumerators the glue exposes (src/faiss_extension.cpp:58-68) */
#define MVS_METRIC_INNER_PRODUCT 0
#define MVS_METRIC_L2 1
#define MVS_METRIC_L1 2
#define MVS_METRIC_Linf 3
#define MVS_METRIC_Lp 4
#define MVS_METRIC_Canberra 20
#define MVS_METRIC_BrayCurtis 21
#define MVS_METRIC_JensenShannon 22
#define MVS_METRIC_Jaccard 23

/* dynamic_cast targets of the glue (src/faiss_extension.cpp:127,133,671,675,691,704; gpu.cpp:69) */
#define MVS_KIND_FLAT 1    /* faiss::IndexFlat / IndexFlatL2 / IndexFlatIP */
#define MVS_KIND_IDMAP 2   /* faiss::IndexIDMap                            */
#define MVS_KIND_IVFFLAT 3 /* faiss::IndexIVFFlat (an IndexIVF)            */
#define MVS_KIND_HNSW 4    /* faiss::IndexHNSWFlat (an IndexHNSW)          */
#define MVS_KIND_PQ 5      /* faiss::IndexPQ (:704), 8 bits per code       */
#define MVS_KIND_IVFPQ 6   /* faiss::IndexIVFPQ (an IndexIVF, :675)        */
#define MVS_KIND_SQ 7      /* faiss::IndexScalarQuantizer, QT_8bit         */
#define MVS_KIND_IVFSQ 8   /* faiss::IndexIVFScalarQuantizer (an IndexIVF) */
#define MVS_KIND_HNSWSQ 9  /* faiss::IndexHNSWSQ, QT_8bit (an IndexHNSW)       */
#define MVS_KIND_REFINE 10 /* faiss::IndexRefineFlat (an IndexRefine)          */
#define MVS_KIND_PRETRANSFORM 11 /* faiss::IndexPreTransform                      */

/* faiss::VectorTransform kinds of a pre-transform chain (mvs_index_pretransform_info) */
#define MVS_VT_LINEAR 0 /* faiss::LinearTransform: a plain matrix, set or loaded ("LTra", "rrot") */
#define MVS_VT_PCA 1    /* faiss::PCAMatrix ("PCA<o>", "PCAW<o>"; "PCAm" / "PcAm")                */
#define MVS_VT_NORM 2   /* faiss::NormalizationTransform, norm 2 ("L2norm"; "VNrm")               */

#define MVS_SEL_NONE 0
#define MVS_SEL_BITMAP 1 /* faiss::IDSelectorBitmap(n_bytes, bitmap)  src/faiss_extension.cpp:959  */
#define MVS_SEL_BATCH 2  /* faiss::IDSelectorBatch(n, ids)            src/faiss_extension.cpp:1008 */
#define MVS_SEL_PROGRAM 3 /* a postfix program of mvs_sel_node: the other classes of faiss/impl/IDSelector.h ("selector programs" below) */

typedef struct mvs_index mvs_index;

/* faiss::SearchParameters / SearchParametersIVF / SearchParametersHNSW as built by
 * innerCreateSearchParameters (src/faiss_extension.cpp:668-721).  Zero = FAISS default. */
typedef struct mvs_search_params {
	int64_t nprobe;       /* SearchParametersIVF::nprobe   (:683-686), default 1  */
	int64_t efSearch;     /* SearchParametersHNSW::efSearch (:696-699), default 16; for IVF<n>_HNSW<m> the efSearch of
	                         the coarse quantizer's SearchParametersHNSW (quantizer_params, :679-681) */
	int32_t sel_kind;     /* MVS_SEL_*; SearchParameters::sel (:678,:694,:719)     */
	int32_t reserved;
	const void *sel_data; /* bitmap bytes | int64 ids | mvs_sel_node array; HOST memory owned by the caller */
	int64_t sel_n;        /* bitmap: bytes; batch: number of ids; program: number of nodes */
} mvs_search_params;

/* faiss::FaissException::msg / what()  -- src/faiss_extension.cpp:397,514,584,632 */
const char *mvs_last_error(void);

/* faiss::index_factory(d, description, metric)  -- src/faiss_extension.cpp:154-155.
 * The index is created device-native on the device named by env MVS_DEVICE (default 0). */
int mvs_index_factory(mvs_index **out, int d, const char *description, int metric);
/* ~Index (unique_ptr<faiss::Index> dropped by ObjectCache)  -- src/faiss_extension.cpp:264 */
void mvs_index_free(mvs_index *ix);

/* Index::d / ntotal / is_trained / metric_type  -- src/faiss_extension.cpp:159,355,490,518 */
int mvs_index_d(const mvs_index *ix);
int64_t mvs_index_ntotal(const mvs_index *ix);
int mvs_index_is_trained(const mvs_index *ix);
int mvs_index_metric_type(const mvs_index *ix);
/* the glue's dynamic_cast to IndexIDMap / IndexIVF / IndexHNSW -- returns MVS_KIND_* */
int mvs_index_kind(const mvs_index *ix);
/* IndexIDMap::index (:129,:673) ; IndexIVF::quantizer (:680).  Borrowed pointers, NULL if n/a. */
mvs_index *mvs_index_idmap_sub(mvs_index *ix);
mvs_index *mvs_index_ivf_quantizer(mvs_index *ix);
/* IVF introspection (IndexIVF::nlist, quantizer centroids): lets parity tests share centroids with the oracle */
int64_t mvs_index_ivf_nlist(const mvs_index *ix);
int mvs_index_ivf_get_centroids(mvs_index *ix, float *out /* nlist*d */);
int mvs_index_ivf_set_centroids(mvs_index *ix, const float *centroids /* nlist*d; marks trained */);
/* IndexHNSW::hnsw.efConstruction = v  -- src/faiss_extension.cpp:136-139 */
int mvs_index_hnsw_set_ef_construction(mvs_index *ix, int v);
/* the value the next add will build with (IDMap wrappers are looked through); -1 if the index is not HNSW */
int mvs_index_hnsw_get_ef_construction(mvs_index *ix);
/* HNSW introspection (HNSW::levels / offsets / neighbors, FAISS's flat layout: 2M slots at level 0, M above, -1 =
 * empty): lets parity tests compare the device-built graph with the oracle's.  graph_info returns the number of
 * neighbour slots (offsets[ntotal]) or -1 if the index is not an HNSW index. */
int64_t mvs_index_hnsw_graph_info(mvs_index *ix, int *max_level, int *entry_point);
/* measurement only (bench.py): counters of the last search run with kernel timing on -- distance evaluations (what FAISS's walk
   evaluates: the algorithmic unit of SURVEY 8d), f32 rows actually fetched, bf16 rows looked at first (csrc/hnsw.hip, "bf16 first look") */
int mvs_index_hnsw_walk_stats(mvs_index *ix, double *evaluations, double *f32_rows, double *bf16_rows);
int mvs_index_hnsw_get_graph(mvs_index *ix, int32_t *levels /* ntotal */, int64_t *offsets /* ntotal+1 */,
                             int32_t *neighbors /* offsets[ntotal] */);

/* ---- product-quantised indexes: "PQ<M>" / "PQ<M>x8", alone or under "IDMap," / "IDMap2," -- the faiss::IndexPQ that
 * innerCreateSearchParameters casts to (src/faiss_extension.cpp:704; it builds a SearchParametersPQ and sets NO selector, :706).
 * FAISS's own IndexPQ results depend on its SIMD build and heap layout; THESE RULES are the contract (DESIGN.md "PQ"):
 *   geometry  dsub = d / M, ksub = 256.  d % M != 0: "... multiple of the number of subquantizers (M)".  PQ<M>x<b>, b != 8, and
 *             M > 128: "This index type is not implemented on the MI355X path yet: ...".  L2 and inner product only.
 *   train     codebook m = the centroids "IVF256,Flat" (L2) learns from columns [m dsub, (m+1) dsub) of x (ProductQuantizer::train:
 *             one Clustering(dsub, 256) per sub-space; L2 k-means also under inner product).  n < 256: "... should be at least as
 *             large as number of clusters ..." (:400,:592).  add before train fails ('is_trained').  train again is accepted while
 *             ntotal == 0 and REJECTED afterwards (FAISS would retrain and leave the stored codes stale).
 *   add       code[i][m] = the j minimising acc = fmaf(t, t, acc), t = x[k] - c_j[k], k ascending over the sub-vector; the
 *             smallest j on a tie; independent of the batch.  add_with_ids on a bare PQ<M>: "add_with_ids not implemented ..." (:523)
 *   search    T[q][m][j] = that chain (L2) or acc = fmaf(x[k], c_j[k], acc) (inner product) between query sub-vector m and centroid
 *             j; dis(q, i) = ((T[q][0][c_i0] + T[q][1][c_i1]) + ...) + T[q][M-1][c_i,M-1] in f32.  The k best in the PURE order:
 *             distance ascending (L2) / descending (inner product), equal distances by ascending internal row; missing slots are
 *             label -1 with FLT_MAX / -FLT_MAX.  1 <= k <= 2048.  Under IDMap labels are id_map[row]; ties still order by row.
 *   admission the k best are taken among the values FAISS's heap can hold (also IVF<n>,PQ<M>, SQ8, IVF<n>,SQ8 below): the heap starts full
 *             of (neutral, -1), neutral = FLT_MAX (L2) / -FLT_MAX (inner product), and takes a value only if it is STRICTLY better than
 *             its worst in a float comparison.  So a NaN score is never a result, nor is +inf (an overflowed sum) or FLT_MAX under L2, nor
 *             -inf or -FLT_MAX under inner product: such slots are missing slots, label -1 with FLT_MAX / -FLT_MAX, never id_map[...].
 *             +inf under inner product is admitted and is the best value.  Queries are not checked: a NaN or inf component is input.
 *   selectors MVS_SEL_BITMAP / MVS_SEL_BATCH are honoured in the scan (the external id under IDMap); a rejected row enters no list.
 *             (The reference glue itself never passes one to a PQ index: :706.)
 *   placement to_gpu / clone_to_gpu(device >= 0) / write_index / read_index (fourcc "IxPq") work; sharding (clone_to_gpu(-1),
 *             mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented" (gpu.cpp:52).
 * mvs_index_get_stat: "pq_query_block" = queries whose tables one scan workgroup holds, "pq_rows_per_workgroup" = rows it walks
 * (workgroup edges are at multiples of it), "pq_scan_launches" / "pq_scan_rescans" = scan launches of the last search / of those,
 * ranges scanned again in halves after a candidate bucket overflowed. */
/* ProductQuantizer::M / nbits of the IndexPQ the glue casts to (:704); IDMap wrappers are looked through */
int mvs_index_pq_info(const mvs_index *ix, int *M, int *nbits);
/* ProductQuantizer::centroids [M][256][d / M] (no counterpart in the glue: lets parity tests share codebooks with the CPU model) */
int mvs_index_pq_get_centroids(mvs_index *ix, float *out /* M*256*dsub */);
/* the same, inwards: marks the index trained; only while ntotal == 0 (no counterpart in the glue) */
int mvs_index_pq_set_centroids(mvs_index *ix, const float *centroids /* M*256*dsub */);
/* IndexPQ::codes rows [row0, row0 + n) (no counterpart in the glue) */
int mvs_index_pq_get_codes(mvs_index *ix, int64_t row0, int64_t n, uint8_t *out /* n*M */);

/* ---- inverted lists of product-quantised residuals: "IVF<n>,PQ<M>" / "IVF<n>,PQ<M>x8", alone or under "IDMap," / "IDMap2," -- a
 * faiss::IndexIVFPQ, i.e. an IndexIVF: the glue's dynamic_cast<faiss::IndexIVF *> (src/faiss_extension.cpp:675) succeeds and sets nprobe;
 * its dynamic_cast<faiss::IndexPQ *> (:704) does not.  MVS_KIND_IVFPQ.  As for PQ<M>, FAISS's own results depend on its SIMD build, its
 * precomputed-table mode and its heap layout; THESE RULES are the contract:
 *   strings   L2 and inner product; M <= 128, d % M == 0, 8 bits per code, 1 <= k <= 2048.  "IVF<n>_HNSW<m>,PQ<M>", "PQ<M>x<b>" with
 *             b != 8, M > 128 and "OPQ..." prefixes: "This index type is not implemented on the MI355X path yet: ...".  d % M != 0:
 *             PQ's message.
 *   accessors mvs_index_ivf_quantizer / _ivf_nlist / _ivf_get_centroids / _ivf_set_centroids and mvs_index_pq_info / _pq_get_centroids /
 *             _pq_set_centroids accept the kind; mvs_index_pq_get_codes stays IndexPQ-only (the codes live in the lists).
 *   train     1. the coarse centroids are exactly what "IVF<n>,Flat" of the same metric learns from x (spherical under inner product),
 *             held by an own Flat quantiser.  2. every training row goes to a list by the quantiser's k = 1 search -- the call add
 *             makes --; its residual is r[k] = x[k] - c[k], one f32 subtraction per component.  3. codebook m = what "IVF256,Flat" (L2)
 *             learns from columns [m dsub, (m+1) dsub) of ALL n residuals in input order (L2 k-means also under inner product; any
 *             subsampling is the k-means' own).  n < nlist or n < 256: "... at least as large as number of clusters ...".  Training
 *             again is accepted while ntotal == 0 and rejected afterwards.  ivf_set_centroids + pq_set_centroids mark the index
 *             trained without k-means: it is trained once both are present.  by_residual is always true, under both metrics.
 *   add       list = the quantiser's k = 1 label; code = PQ's encoding rule on the residual (the pair-path L2 chain, smallest j on a
 *             tie); rows are appended to their list in arrival order, independent of the batches.  Stored id = the add_with_ids id, or
 *             label_offset + sequence number, as for IVF<n>,Flat; under IDMap labels are id_map[row].  add before train fails
 *             ('is_trained').  At most 2^31 - 1024 rows.
 *   search    the probed lists of a query x are what the quantiser returns for k = min(nprobe, nlist), in its order (probe rank 0, 1,
 *             ...; a -1 entry is skipped).  For the pair (query, probed list with centroid c):
 *               L2             v = x - c (one f32 subtraction per component); T[m][j] = the chain acc = fmaf(t, t, acc),
 *                              t = v[m dsub + k] - cb[m][j][k], k ascending from +0; dis = ((T[0][code0] + T[1][code1]) + ...) in f32
 *               inner product  v = x; T[m][j] = the chain acc = fmaf(v[m dsub + k], cb[m][j][k], acc); base = the chain
 *                              acc = fmaf(x[k], c[k], acc) over all d, k ascending -- computed by the scan, NOT the quantiser's reported
 *                              distance --; dis = (((base + T[0][code0]) + T[1][code1]) + ...)
 *             The k best in the PURE order: distance (L2 ascending, inner product descending), then probe rank, then position in the
 *             list -- among the values the admission rule of PQ<M> (above) lets in; a list whose coarse value that rule refuses is a -1
 *             probe; missing slots are label -1 with FLT_MAX / -FLT_MAX.  nprobe comes from the search parameters, else the index's own
 *             value (default 1).
 *   selectors MVS_SEL_BITMAP / MVS_SEL_BATCH are tested in the scan on the stored id (the external id under IDMap); a rejected row
 *             enters no list.
 *   placement to_gpu / clone_to_gpu(device >= 0) / write_index / read_index (fourcc "IwPQ") go through the host image; sharding
 *             (clone_to_gpu(-1), mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented".
 * mvs_index_get_stat: "ivfpq_pair_block" = (query, list) pairs whose tables one scan workgroup holds, "ivfpq_rows_per_workgroup" = rows
 * of a list it walks = entries of a query's candidate bucket, "ivfpq_scan_launches" / "ivfpq_scan_rescans" = scan launches of the last
 * search / of those, units scanned again in halves after a bucket overflowed. */
/* rows of inverted list list_no (ArrayInvertedLists::list_size); -1 and mvs_last_error on another kind; IDMap wrappers are looked through */
int64_t mvs_index_ivfpq_list_size(const mvs_index *ix, int64_t list_no);
/* the list's stored ids and codes in list order (InvertedLists::get_ids / get_codes); either pointer may be NULL */
int mvs_index_ivfpq_get_list(mvs_index *ix, int64_t list_no, int64_t *ids /* size */, uint8_t *codes /* size*M */);

/* ---- 8-bit scalar-quantised indexes: "SQ8" (faiss::IndexScalarQuantizer, MVS_KIND_SQ) and "IVF<n>,SQ8" (faiss::IndexIVFScalarQuantizer,
 * MVS_KIND_IVFSQ: an IndexIVF, so the glue's dynamic_cast<faiss::IndexIVF *> (src/faiss_extension.cpp:675) succeeds and sets nprobe), alone
 * or under "IDMap," / "IDMap2,".  One byte per component, 4 x smaller than Flat; FAISS's own SQ results depend on its SIMD build and heap
 * layout; THESE RULES are the contract:
 *   strings   L2 and inner product; 1 <= d <= 2048; 1 <= k <= 2048.  "SQ4", "SQ6", "SQfp16", "SQ8_direct" and every other qtype,
 *             "IVF<n>_HNSW<m>,SQ8" and d > 2048: "This index type is not implemented on the MI355X path yet: ...".
 *   no contraction   every operation below is ONE IEEE f32 operation, rounded on its own: a + b * c is a multiplication and an addition,
 *             never an fma; only the chains written fmaf are fused.
 *   train     vmin[k] / vmax[k] = the minimum / maximum of component k over all n training rows, vdiff[k] = vmax[k] - vmin[k].  For
 *             IVF<n>,SQ8: first the coarse centroids, exactly what "IVF<n>,Flat" of the same metric learns from x (an own Flat quantiser);
 *             then every training row goes to a list by the quantiser's k = 1 search and min / max are taken over the residuals
 *             r[k] = x[k] - c[k].  by_residual is always true, under both metrics.  n < nlist: "... at least as large as number of clusters
 *             ..."; n = 0 fails.  Training again is accepted while ntotal == 0 and rejected afterwards.  Derived once, at training:
 *             s[k] = vdiff[k] / 255.0f and a[k] = vmin[k] + 0.5f * s[k].  (min / max do not depend on the order: vmin and vdiff equal a
 *             numpy reduction as VALUES; the sign of a zero minimum is not specified.)
 *   encode    of the row value y (x[k], or the residual): code 0 if vdiff[k] == 0; else xi = (y - vmin[k]) / vdiff[k] clamped to [0, 1]
 *             and code = (int)(255.0f * xi), truncating.  Independent of the add batches.  IVF: list = the quantiser's k = 1 label; rows
 *             are appended to their list in arrival order.  add before train fails ('is_trained').  add_with_ids on a bare SQ8:
 *             "add_with_ids not implemented ..." (:523).  At most 2^31 - 1024 rows.
 *   decode    dec(c, k) = a[k] + (float)c * s[k]: one multiplication, one addition.
 *   distance  SQ8, L2: the chain acc = fmaf(t, t, acc), t = x[k] - dec(code[k], k), k ascending from +0.  SQ8, inner product: the chain
 *             acc = fmaf(x[k], dec, acc).  IVF<n>,SQ8, L2: the same chain with v[k] = x[k] - c[k] in place of x (c: the probed list's
 *             centroid).  IVF<n>,SQ8, inner product: dis = base + t; base = the chain acc = fmaf(x[k], c[k], acc) over all d -- computed by
 *             the scan, NOT the quantiser's reported distance --, t = the chain acc = fmaf(x[k], dec, acc) from +0; then one f32 addition.
 *   order     the k best in the PURE order among the values the admission rule of PQ<M> (above) lets in -- no NaN, nothing that is not
 *             strictly better than FLT_MAX (L2) / -FLT_MAX (inner product).  SQ8: distance, then internal row.  IVF<n>,SQ8: distance, then probe rank, then position in
 *             the list.  L2 ascending, inner product descending; missing slots are label -1 with FLT_MAX / -FLT_MAX.  The probed lists are
 *             the quantiser's answer for k = min(nprobe, nlist), in its order; a -1 entry is skipped.  Stored ids, label_offset and IDMap
 *             behave as for IVF<n>,PQ<M>.
 *   selectors MVS_SEL_BITMAP / MVS_SEL_BATCH are tested in the scan on the stored id (the external id under IDMap); a rejected row
 *             enters no list.
 *   placement to_gpu / clone_to_gpu(device >= 0) / write_index / read_index (fourcc "IxSQ" / "IwSq") go through the host image; sharding
 *             (clone_to_gpu(-1), mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented".
 *   accessors mvs_index_ivf_quantizer / _ivf_nlist / _ivf_get_centroids / _ivf_set_centroids accept MVS_KIND_IVFSQ.
 * mvs_index_get_stat: "sq_pair_block" = (query, list) pairs one scan workgroup serves, "sq_rows_per_workgroup" = positions of a list it
 * walks = entries of a query's candidate bucket, "sq_scan_launches" / "sq_scan_rescans" = scan launches of the last search / of those,
 * units scanned again in halves after a bucket overflowed, "sq_device_bytes" = device memory of the code stores, ids and range. */
/* ---- HNSW over 8-bit scalar-quantised rows: "HNSW<M>,SQ8" / "HNSW<M>_SQ8" (faiss::IndexHNSWSQ, MVS_KIND_HNSWSQ: an IndexHNSW, so the glue's
 * dynamic_cast<faiss::IndexHNSW *> (src/faiss_extension.cpp:133 and :691) reaches it: efConstruction, efSearch and selectors work as for
 * "HNSW<M>"), alone or under "IDMap," / "IDMap2,".  One code byte per component instead of the f32 row and its bf16 copy.  As for SQ8, FAISS's
 * own bits depend on its SIMD build and thread interleaving; THESE RULES are the contract:
 *   strings   "HNSW<M>,SQ8" and "HNSW<M>_SQ8"; a bare "HNSW,SQ8" means M = 32.  L2 and inner product; 1 <= d <= 2048; M as for "HNSW<M>".
 *             "HNSW<M>,SQ4", "HNSW<M>,PQ<m>", every other suffix and d > 2048: "This index type is not implemented on the MI355X path yet:
 *             ...".  "HNSW<M>" and "HNSW<M>,Flat" are unchanged in every bit.
 *   train     is_trained is false at creation.  train(n, x) learns exactly SQ8's range: vmin[k] and vdiff[k] over the n rows, no
 *             residuals; s = vdiff / 255.0f and a = vmin + 0.5f * s, each ONE IEEE f32 operation.  n = 0 fails with SQ8's message.  Training
 *             again is accepted while ntotal == 0 and rejected afterwards; mvs_index_sq_set_trained marks the index trained.  add before
 *             train fails ('is_trained'); add_with_ids on the bare index: "add_with_ids not implemented for this type of index".
 *   encode    SQ8's rule, verbatim: code = (int)(255.0f * clamp((x - vmin) / vdiff, 0, 1)), 0 where vdiff == 0.
 *   decode    dec(c, k) = a[k] + (float)c * s[k]: one multiplication and one addition, never an fma.
 *   graph, search   the index IS "HNSW<M>" over the decoded rows y_i = dec(enc(x_i)): levels, insertion order, efConstruction, neighbour
 *             selection, links, the level-0 walk, efSearch, selectors on results only and the negated inner product are what "HNSW<M>" does
 *             when it is handed the rows y.  The query of an insertion is the point's own DECODED row; search queries are the caller's f32
 *             vectors.  The distance is the canonical HNSW arithmetic (oracle/orc_hnsw.c dc_q: lane (k / 4) % 64 holds component k, four
 *             fmaf chains per lane, a fixed reduction tree) with y in place of the stored f32 row.
 *             DIFFERENCE FROM FAISS: faiss::IndexHNSWSQ inserts with the RAW row as the query.  Inserting with the decoded row makes the
 *             graph a function of the stored codes alone.
 *   concurrency   with option hnsw_build_waves = 1 graph, labels and distances equal the model bit for bit; with the default concurrent
 *             build only recall is comparable, as for "HNSW<M>".
 *   storage   one code row of dp = ceil(d / 4) * 4 bytes per vertex, zero padded; no f32 store and no bf16 copy: the bf16 first look does
 *             not apply and option hnsw_bf16 is ignored.  mvs_index_hnsw_walk_stats reports the code rows fetched in f32_rows and 0 in
 *             bf16_rows.
 *   placement write_index / read_index: fourcc "IHNs" = the header and the HNSW block exactly as "IHNf" writes them, then the storage as
 *             an "IxSQ" image (qtype 0, range, codes).  "IHNs" with a Flat storage and "IHNf" with an SQ storage are refused on reading.  An
 *             image is adopted as it is: range and codes are not encoded again.  clone_to_gpu(device >= 0) goes through the host image;
 *             to_gpu(device) is what it is for "HNSW<M>" (nothing to do on the index's own device, refused for another one); sharding (clone_to_gpu(-1), mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented".
 *   accessors every mvs_index_hnsw_* function accepts both HNSW kinds; mvs_index_sq_get_trained / _sq_set_trained / _sq_get_codes accept
 *             MVS_KIND_HNSWSQ (codes in vertex order, d bytes per row).
 * mvs_index_get_stat, both HNSW kinds: "hnsw_row_bytes" = the bytes one distance evaluation reads from the store (dp for this kind, 4 dp for
 * "HNSW<M>"), "hnsw_store_bytes" = the device bytes of every row store the index holds now (the codes, or the f32 rows plus the bf16 copy). */
/* ScalarQuantizer::trained as vmin [d] | vdiff [d] (no counterpart in the glue: lets parity tests share the range with the CPU model);
 * IDMap wrappers are looked through, here and below */
int mvs_index_sq_get_trained(mvs_index *ix, float *out /* 2*d */);
/* the same, inwards: marks a bare SQ8 trained; an IVF<n>,SQ8 is trained once this and mvs_index_ivf_set_centroids are both present;
 * only while ntotal == 0 */
int mvs_index_sq_set_trained(mvs_index *ix, const float *trained /* 2*d */);
/* IndexScalarQuantizer::codes rows [row0, row0 + n); SQ8 and HNSW<M>,SQ8 only (the IVF kind's codes live in the lists) */
int mvs_index_sq_get_codes(mvs_index *ix, int64_t row0, int64_t n, uint8_t *out /* n*d */);
/* rows of inverted list list_no (ArrayInvertedLists::list_size); -1 and mvs_last_error on another kind */
int64_t mvs_index_ivfsq_list_size(const mvs_index *ix, int64_t list_no);
/* the list's stored ids and codes in list order (InvertedLists::get_ids / get_codes); either pointer may be NULL */
int mvs_index_ivfsq_get_list(mvs_index *ix, int64_t list_no, int64_t *ids /* size */, uint8_t *codes /* size*d */);

/* ---- exact f32 re-ranking over the quantised indexes: "<base>,RFlat" / "<base>,Refine(Flat)" (faiss::IndexRefineFlat, MVS_KIND_REFINE), alone
 * or under "IDMap," / "IDMap2," -- the order is IDMap(Refine(base)), as FAISS parses it.  The index owns two sub-indexes of equal d and
 * metric: the BASE, one of the four scanning kinds, and the STORE, a Flat index holding the same rows in arrival order; the store is never
 * searched.  THESE RULES are the contract:
 *   strings   <base> is "PQ<M>[x8]", "IVF<n>,PQ<M>[x8]", "SQ8" or "IVF<n>,SQ8"; L2 and inner product only.  Every other base ("Flat",
 *             "IVF<n>,Flat", every "HNSW..."), whatever the base's own maker refuses, every other refine store ("Refine(SQ8)", ...) and a
 *             second refine stage: "This index type is not implemented on the MI355X path yet: ...".
 *   train     trains the base; is_trained is the base's.
 *   add       requires is_trained (the base's 'is_trained' failure).  The base's add runs first, without ids and with its label_offset held
 *             at 0; the store's add runs second: if the base throws, the store is unchanged.  For the IVF bases the stored id of a row is
 *             therefore its row number in the store.  ntotal is the store's.  add_with_ids on the bare index: "add_with_ids not implemented
 *             for this type of index".  Device-resident adds do the same.
 *   k_factor  a float, default 1, k_factor >= 1 (mvs_index_refine_set_k_factor / _get_k_factor; IDMap wrappers are looked through).
 *   search    kb = (int64)((float)k * k_factor): an f32 product, truncated.  kb > 2048 fails, naming k, k_factor and the limit; k <= 0 fails
 *             as the bases do.  The base is searched for kb entries with the caller's whole mvs_search_params: nprobe, and the selector
 *             honoured in the base's scan (under IDMap the selector tests the external id).  Every candidate with store row r >= 0 gets
 *             the pair-path chain from +0, j ascending over the d logical components -- L2: acc = fmaf(t, t, acc), t = x[j] - y_r[j];
 *             inner product: acc = fmaf(x[j], y_r[j], acc) -- which is what FAISS's fvec_L2sqr / fvec_inner_product restate; a -1 candidate
 *             is skipped.  Result: the k best candidates in the PURE order -- exact value ascending (L2) / descending (inner product), equal
 *             values by ascending store row --; missing slots are label -1 with FLT_MAX / -FLT_MAX.  Labels are label_offset + row, or
 *             id_map[row] under IDMap.
 *             DIFFERENCES FROM FAISS: ties follow rows, not FAISS's heap; the parameters go to the base whole, whereas FAISS wants an
 *             IndexRefineSearchParameters (k_factor plus the base's parameters).
 *   options   mvs_index_set_option forwards to the base.
 *   placement write_index / read_index: fourcc "IxRF" = the index header, the base's image, the store's image ("IxF2" / "IxFI"), then
 *             float k_factor -- the order FAISS's index_write.cpp uses for IndexRefine, RESTATED FROM MEMORY: no FAISS source was at hand.
 *             Reading refuses an image whose base and store disagree in d, metric or ntotal, whose IVF base holds a stored id outside
 *             [0, ntotal), or whose second index is not a Flat image.  clone_to_gpu(device >= 0) and to_gpu go through the host image;
 *             sharding (clone_to_gpu(-1), mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented".
 * mvs_index_get_stat: "refine_candidates" = kb of the last search, "refine_store_bytes" = device bytes of the store's f32 rows,
 * "refine_query_chunk" = queries per pass of the last search (the base's candidate lists, 12 bytes an entry, stay within 256 MB); every
 * other name goes to the base. */
/* IndexRefine::base_index / refine_index.  Borrowed pointers, NULL if the index is not a Refine index; IDMap wrappers are looked through.
 * The pq_* / ivf_* / sq_* accessors take the base handle: parity tests share codebooks, centroids and ranges with the CPU models */
mvs_index *mvs_index_refine_base(mvs_index *ix);
mvs_index *mvs_index_refine_store(mvs_index *ix);
/* IndexRefine::k_factor; set fails for k_factor < 1 (or NaN) and on another kind */
int mvs_index_refine_set_k_factor(mvs_index *ix, float k_factor);
int mvs_index_refine_get_k_factor(mvs_index *ix, float *k_factor);

/* ---- pre-transform indexes: "<t1>,...,<tn>,<sub>" (faiss::IndexPreTransform, MVS_KIND_PRETRANSFORM), n = 1 to 4, alone or under "IDMap," /
 * "IDMap2," -- the order is IDMap(PreTransform(sub)), as FAISS parses it.  The index owns a chain of vector transforms and ONE sub-index of
 * any other kind at the chain's output dimension; d is the chain's input dimension, the metric the sub-index's.  THESE RULES are the
 * contract:
 *   strings   <t> is "PCA<o>", "PCAW<o>" or "L2norm"; <sub> is any string the factory accepts at the resulting dimension except a refine
 *             suffix; 1 <= o <= d_in <= 2048 ("PCA<o>" with o > d_in fails, naming both).  "PCAR<o>", "PCAWR<o>", "RR<o>", "ITQ<o>",
 *             "Pad<o>", "LDA<o>": "This index type is not implemented on the MI355X path yet: <full string>".  Every "OPQ..." string and
 *             "<chain>,<base>,RFlat" keep their refusals; a chain with no sub-index ("PCA4") is "could not parse index string".
 *   linear    A [d_out][d_in] in f32 and, if have_bias, b [d_out]: y[j] = (the chain acc = fmaf(x[k], A[j][k], acc), k ascending from +0)
 *             + b[j].  The bias is ONE f32 addition after the chain, and it is absent without a bias.  FAISS does an sgemm with beta = 1,
 *             whose order BLAS does not define; these rules are the contract.  pretransform_apply_kernel runs on v_mfma_f32_32x32x2_f32,
 *             bit for bit that chain.
 *   L2norm    nr = the chain acc = fmaf(x[k], x[k], acc) from +0; if nr > 0: inv = 1.0f / sqrtf(nr), both correctly rounded, and
 *             y[k] = x[k] * inv; otherwise the row is copied (FAISS's fvec_renorm_L2).  Only norm 2 is supported.
 *   PCA       training is deterministic (fixed partitions, fixed reduction trees, no floating-point atomics): training twice on the same
 *             rows gives the same bits.  mean and C = (X - mean)^T (X - mean) / n in f64 from all n rows; eigenpairs of C in f64 by a
 *             one-sided Jacobi method on the device, until every normalised off-diagonal product is <= 1e-12, at most 30 sweeps (else it
 *             fails with a message); eigenvalues descend; each eigenvector's sign makes its component of largest magnitude positive, the
 *             first such on a tie (a stated DEPARTURE: FAISS leaves the sign to LAPACK); PCAMat [d_in][d_in] and eigenvalues [d_in] are
 *             the f64 values rounded once to f32; A = the first d_out rows; for PCAW each row is scaled in f64 by
 *             (lambda_i + epsilon)^(-1/2), lambda_i the f64 eigenvalue, before the one rounding, epsilon = 0, and lambda_i <= 0 fails;
 *             b[j] = -sum_k A[j][k] mean[k], accumulated in f64 over the f32 values with k ascending, and rounded once.  n < d_out fails
 *             naming n and d_out; n = 0 fails.
 *   train     each transform that is not yet trained is trained on the output of those before it; a transform that is already trained is
 *             left alone (FAISS's rule); then the sub-index, unless it is trained already, trains on the transformed rows.  is_trained =
 *             all transforms trained and the sub-index trained.
 *   add       add / add_with_ids and their device variants transform the rows, then forward them; a bare sub-index that refuses ids
 *             refuses with its own text.  Adds are transformed in chunks whose workspace stays within 256 MB; results do not depend on the
 *             chunking or on the add batches, except where the sub-index's own build depends on its add batches (HNSW<M>, as FAISS's:
 *             a chunk reaches it as one batch).  An untrained chain fails with 'is_trained'.
 *   search    search / search_device transform the queries (in one piece), then forward them with the caller's mvs_search_params whole:
 *             nprobe, efSearch and selector.  Labels, distances, ties, k limits and label_offset are the sub-index's, in the transformed
 *             space; under IDMap the id map goes through.  Kernel info and kernel timing remain the sub-index's.  range_search and
 *             remove_ids forward the same way; a sub-index kind that refuses them refuses with its own text.
 *   refusals  the reconstruct family refuses with FAISS's base-class text (the reverse transform is out of scope); sharding
 *             (clone_to_gpu(-1), mvs_index_shard_to_gpus, MVS_DEVICES) fails with "This index type is not implemented".
 *   placement to_gpu and clone_to_gpu(device >= 0) go through the host image; mvs_index_set_option forwards to the sub-index.
 *   files     fourcc "IxPT": the index header, int32 n, n transforms, the sub-index's image -- FAISS's layout RESTATED FROM MEMORY: no
 *             FAISS source was at hand.  One transform: its fourcc; for PCA float eigen_power, float epsilon ("PcAm" only; the old "PCAm"
 *             lacks it), 1-byte random_rotation, int32 balanced_bins, the vectors mean, eigenvalues, PCAMat; for every linear kind 1-byte
 *             have_bias, vector A, vector b; for "VNrm" float norm; for all int32 d_in, int32 d_out, 1-byte is_trained.  Written: PCA and
 *             PCAW as "PcAm", L2norm as "VNrm", a set or loaded plain matrix as "LTra".  Read: "LTra", "rrot", "PCAm" and "PcAm" are all
 *             served as linear transforms (PCA's extra vectors are kept for writing back), so a file FAISS wrote for "OPQ...,IVF...,PQ..."
 *             is served; "VNrm" with norm 2; every other transform fourcc is refused by name.  Refused with a message: A whose size is not
 *             d_in * d_out, b whose size is not d_out when have_bias is set, chain dimensions that do not join, a chain whose output
 *             dimension is not the sub-index's d, a norm other than 2, a truncated file.
 * mvs_index_get_stat: "pretransform_apply_launches" = kernel launches of the last call's transforms, "pretransform_workspace_bytes" = the
 * workspace it held; every other name goes to the sub-index, as do mvs_index_prefilter_stats, mvs_index_collect_stats,
 * mvs_index_shadow_stats and mvs_index_ivf_probe_stats: the searching kernels are the sub-index's. */
/* IndexPreTransform::index.  A borrowed pointer, NULL if the index is not a PreTransform index; IDMap wrappers are looked through (as by
 * every function below).  The ivf_* / pq_* / sq_* accessors take it: parity tests share centroids, codebooks and ranges with the CPU models */
mvs_index *mvs_index_pretransform_sub(mvs_index *ix);
/* IndexPreTransform::chain.size(); -1 on another kind */
int mvs_index_pretransform_count(const mvs_index *ix);
/* transform i: its MVS_VT_* type, dimensions, have_bias (0 for a normalisation) and is_trained; any pointer may be NULL */
int mvs_index_pretransform_info(const mvs_index *ix, int i, int *type, int *d_in, int *d_out, int *have_bias, int *is_trained);
/* LinearTransform::A / b of a trained linear or PCA transform; b reads as zeros without a bias; either pointer may be NULL */
int mvs_index_pretransform_get_linear(mvs_index *ix, int i, float *A /* d_out*d_in */, float *b /* d_out */);
/* the same, inwards, b NULL for none: marks the transform trained, works only while ntotal == 0, and turns a PCA slot into a plain linear one */
int mvs_index_pretransform_set_linear(mvs_index *ix, int i, const float *A /* d_out*d_in */, const float *b /* d_out or NULL */);
/* PCAMatrix::mean / eigenvalues of a trained PCA transform; either pointer may be NULL */
int mvs_index_pretransform_get_pca(mvs_index *ix, int i, float *mean /* d_in */, float *eigenvalues /* d_in */);
/* IndexPreTransform::apply_chain: n rows of d floats in, n rows of the chain's output dimension out (host / device memory) */
int mvs_index_pretransform_apply(mvs_index *ix, int64_t n, const float *x, float *out);
int mvs_index_pretransform_apply_device(mvs_index *ix, int64_t n, const float *d_x, float *d_out, void *stream);

/* Index::train(n, x)  -- src/faiss_extension.cpp:396,583 */
int mvs_index_train(mvs_index *ix, int64_t n, const float *x);
/* Index::add(n, x)  -- src/faiss_extension.cpp:512,609 */
int mvs_index_add(mvs_index *ix, int64_t n, const float *x);
/* Index::add_with_ids(n, x, ids)  -- src/faiss_extension.cpp:510,607 */
int mvs_index_add_with_ids(mvs_index *ix, int64_t n, const float *x, const int64_t *ids);
/* Index::search(n, x, k, distances, labels, params)  -- src/faiss_extension.cpp:631 */
int mvs_index_search(mvs_index *ix, int64_t n, const float *x, int64_t k, float *distances, int64_t *labels,
                     const mvs_search_params *params);

/* ---- range search: faiss::Index::range_search(n, x, radius, result, params) -- every row within a fixed radius of each query, a
 * variable-length result where search returns a fixed k.  The reference glue never calls it (no call site in src/faiss_extension.cpp);
 * it is the primitive a database extension wants for similarity joins, "all rows with distance < r" and de-duplication.  The hit rule
 * below restates RangeSearchBlockResultHandler / IndexIVF::range_search FROM MEMORY: no FAISS source was at hand.  THESE RULES are the
 * contract:
 *   hit rule  L2: a row is a hit iff dis < radius; inner product: iff dis > radius.  Both are strict.  A NaN radius gives no hit, and a
 *             NaN distance is never a hit: both comparisons are false.
 *   kinds     "Flat" (L2 and inner product), "IVF<n>,Flat" and "IVF<n>_HNSW<m>,Flat", each alone or under "IDMap," / "IDMap2,".  Everything
 *             else -- the other metrics on Flat, "HNSW...", "PQ...", "SQ8", "IVF...,PQ...", "IVF...,SQ8", "...,RFlat", a sharded index --
 *             fails with FAISS's base-class text "range search not implemented".
 *   Flat      dis is exactly what mvs_index_search computes for the same batch (FlatIndex::search_flat's dispatch).  A selector or
 *             n < 20 queries: the per-pair chains -- L2: acc = fmaf(t, t, acc), t = x[k] - y[k]; inner product: acc = fmaf(x[k], y[k], acc),
 *             k ascending from +0.  Otherwise the BLAS-branch value -- L2: (||x||^2 + ||y||^2) - 2 ip in two roundings, clamped at 0, ip and
 *             the norms as k-ordered fma chains; inner product: the chain.  A query's hits are in ascending internal row order; labels are
 *             label_offset + row, or id_map[row] under IDMap; the selector tests the id that search tests (the external id under IDMap).
 *   IVF       the coarse stage is the one search runs for the same mvs_search_params: nprobe 0 means the index's own, clamped to nlist;
 *             efSearch applies to an HNSW quantiser; the Flat quantiser's small-batch / BLAS dispatch is the same.  A query's hits are the
 *             rows of its probed lists whose per-pair chain against the raw row (no residual) passes the rule, ordered by (probe rank,
 *             position in the list).  Labels are the stored ids, or id_map[stored id] under IDMap.  An untrained index fails
 *             ('is_trained').
 *   edges     n == 0: an empty result with lims = [0].  ntotal == 0: all lims are zero.  Rows staged by add() are seen.  A call whose
 *             total hits exceed 2^30 fails with a message naming the count and the radius; nothing is truncated silently.
 *             Ordinals and positions are 32-bit fields: a Flat index of 2^32 rows or IVF lists of 2^31 rows (beyond what add admits) are
 *             refused with a message.
 *   result    lives in HOST memory and belongs to the caller until mvs_range_result_free; query q's hits are entries
 *             [lims[q], lims[q + 1]) of distances and labels.
 * mvs_index_set_option: "range_stream_cap" = entries of the first attempt's hit stream (0: automatic; a scan that overflows it is run once
 * more with the exact size), "range_mfma" = 1 (default) | 0: Flat BLAS-branch batches on the f32 MFMA kernel or on the VALU kernel's formula
 * mode -- same bits.  mvs_index_get_stat "range_rescans" = scans repeated because the stream was too small, over the index's life. */
typedef struct mvs_range_result mvs_range_result;
int mvs_index_range_search(mvs_index *ix, int64_t n, const float *x, float radius, const mvs_search_params *params,
                           mvs_range_result **out);
int64_t mvs_range_result_nq(const mvs_range_result *r);
const int64_t *mvs_range_result_lims(const mvs_range_result *r);      /* nq + 1 */
const float *mvs_range_result_distances(const mvs_range_result *r);   /* lims[nq] */
const int64_t *mvs_range_result_labels(const mvs_range_result *r);    /* lims[nq] */
void mvs_range_result_free(mvs_range_result *r);

/* ---- remove_ids: faiss::Index::remove_ids(const IDSelector &) -- delete rows from an index.  The reference glue never calls it (no call
 * site in src/faiss_extension.cpp) and stock FAISS GPU indexes do not offer it; it is the primitive a database extension needs for DELETE
 * and UPDATE without rebuilding the index from host memory.  The rules below restate IndexFlatCodes::remove_ids, IndexIVF::remove_ids with
 * InvertedLists, IndexIDMap::remove_ids and Index::remove_ids FROM MEMORY: no FAISS source was at hand.  THESE RULES are the contract
 * (DESIGN.md 3.12):
 *   selector  sel_kind is MVS_SEL_BITMAP, MVS_SEL_BATCH or MVS_SEL_PROGRAM ("selector programs" below), host memory owned by the caller;
 *             MVS_SEL_NONE or an unknown kind is an error.
 *             Bitmap: bit `id` is set -- a negative id, or one beyond the bitmap, is not a member.  Batch: `id` occurs in the list;
 *             duplicates in the list and ids that are not in the index are harmless.  n_removed may be NULL.
 *   Flat (any metric), PQ<M>, SQ8   row r is removed iff label_offset + r is a member (the id search's selector tests).  The survivors keep
 *             their relative order and are renumbered 0 .. ntotal'-1: a stable compaction.
 *   IDMap, / IDMap2, over those   row r is removed iff id_map[r] is a member; every row carrying a member id goes (duplicate external ids
 *             are legal).  The rows and id_map compact stably together.
 *   IVF<n>,Flat, IVF<n>_HNSW<m>,Flat, IVF<n>,PQ<M>, IVF<n>,SQ8   work on the STORED id.  Every list is processed on its own by FAISS's
 *             swap-from-the-end loop
 *                 l = size; j = 0; while (j < l) { if member(ids[j]) { --l; ids[j] = ids[l]; codes[j] = codes[l]; } else ++j; }
 *             and then shrinks to l.  j does not advance after a swap, so the order of the survivors inside a list CHANGES: a list with ids
 *             [0,1,2,3,4] and members {0,1} ends as [4,3,2].  That order shows in tie order, in range_search's hit order and in write_index:
 *             it is part of the contract.  Centroids, codebooks, ranges, an HNSW coarse quantiser, nprobe and is_trained are untouched.
 *   IDMap, / IDMap2, over an IVF kind   DEPARTURE FROM FAISS.  The row with stored id s is removed iff id_map[s] is a member; the lists
 *             shrink by the swap rule; id_map compacts stably; every surviving stored id is renumbered to s - #{removed r < s}, so that
 *             id_map[stored id] still names the row's external id.  FAISS leaves the lists' ids as they were and returns wrong labels
 *             afterwards (its documentation restricts IndexIDMap::remove_ids to Flat-like sub-indexes).  If the sub-index's stored ids are
 *             not exactly 0 .. ntotal-1, each once -- only a foreign file can cause it -- the call is refused with a message saying so.
 *   others    HNSW..., HNSW<M>,SQ8, ...,RFlat / ...,Refine(Flat) and a sharded index fail with FAISS's base-class text
 *             "remove_ids not implemented for this type of index"; the index is unchanged.
 *   edges     rows staged by add() are flushed first.  An empty index returns 0, so does an untrained IVF index.  A selector with no member
 *             returns 0 and touches nothing.  Removing every row leaves ntotal = 0: the index is still trained and add works.  A later add()
 *             without ids numbers from the new ntotal, as FAISS does -- on a bare IVF index that can duplicate a stored id (FAISS's
 *             behaviour, kept).  If the allocation for the compacted store fails, the call fails and the index is as before.
 *   after     search (selectors, nprobe, efSearch of an HNSW quantiser), range_search, add / add_with_ids, write_index / read_index,
 *             clone_to_gpu, to_gpu and shard_to_gpus behave bit for bit as on an index built with the surviving rows in the resulting order
 *             and with the resulting stored ids.  (IVF<n>,Flat prints equal distances by stored id: under IDMap an index FILLED AGAIN with
 *             the survivors numbers its stored ids by arrival and agrees in every distance and in every label outside runs of bit-equal
 *             distances; the image written by write_index agrees in every bit.) */
int mvs_index_remove_ids(mvs_index *ix, int32_t sel_kind, const void *sel_data, int64_t sel_n, int64_t *n_removed);

/* ---- merge_from and copy_subset_to: faiss::Index::merge_from(Index &, idx_t add_id), Index::check_compatible_for_merge(const Index &)
 * and IndexIVF::copy_subset_to(IndexIVF &, subset_type_t, idx_t, idx_t) -- rows move between indexes on the device.  They are how an index
 * is built in parallel (every worker fills a private index, the parts are merged at the end) and how an IVF index is split by id.  No row
 * byte passes through host memory: the rows are appended device to device, an IVF kind's host directory is appended, and every list view
 * is derived again on demand.  The rules restate FAISS FROM MEMORY; THESE RULES are the contract:
 *   kinds     merge_from / check_compatible_for_merge: Flat, PQ<M>, SQ8, IVF<n>,Flat, IVF<n>_HNSW<m>,Flat, IVF<n>,PQ<M>, IVF<n>,SQ8, alone or
 *             under IDMap, / IDMap2,.  copy_subset_to: the bare IVF kinds only.  Every other kind -- HNSW..., <base>,RFlat, a pre-transform
 *             chain, a sharded index -- fails with FAISS's base-class texts "merge_from() not implemented" and
 *             "check_compatible_for_merge() not implemented"; both indexes stay untouched.
 *   result    after merge_from(ix, other, add_id) ix is indistinguishable from the index that received ix's rows and then other's rows in
 *             other's arrival order: ntotal, search (labels and distances bit for bit, the order of ties included), range_search, the
 *             reconstruct family, remove_ids, the list getters and the bytes write_index produces.
 *   Flat, PQ<M>, SQ8   other's row i becomes row ntotal_before + i (label: label_offset + that).  add_id must be 0, otherwise the call fails
 *             with FAISS's "cannot set ids in FlatCodes index".
 *   IVF kinds other's entries are appended to the same-numbered lists of ix, behind ix's entries and in other's list order, with stored id +
 *             add_id.  Rows other holds in no list travel as they are.  The codes are other's bytes: nothing is re-encoded or re-assigned.
 *   IDMap     the wrapped indexes merge, then other's id_map[i] + add_id is appended to ix's id map.  DEPARTURE FROM FAISS: an IVF kind
 *             under IDMap resolves labels as id_map[stored id], so its sub-merge shifts other's stored ids by ix's sub-index ntotal (FAISS
 *             passes 0, after which two rows share a stored id and labels go wrong).
 *   other     ends with ntotal == 0: empty lists, an empty id map, an empty store.  It keeps its trained state, centroids, codebooks or
 *             range, nprobe and tuning, and can be added to and merged again.
 *   compatibility   checked before anything changes; the message names the first difference: the same kind (IDMap against IDMap2
 *             differs), d, metric, device, nlist, code size / M, both trained.  DELIBERATELY STRICTER THAN FAISS: coarse centroids, PQ
 *             codebooks and the SQ range must be equal bit for bit (compared on the device; an HNSW coarse quantiser's centroids through
 *             its image).  FAISS merges codes of different codebooks silently, which is never what the caller meant.  other == ix is
 *             refused.  The 2^31-row guard of add applies to the sum.
 *   failure   every allocation that can fail (store growth, id map growth) is made before any state changes: a refused or failed call
 *             leaves both indexes answering as before.
 *   statistic ivf_ids_ascending (mvs_index_get_stat) stays 1 only if both sides had 1 and other's smallest shifted id exceeds ix's largest.
 *   copy_subset_to   ix is unchanged; the selected entries are appended to other's lists with their ids unchanged, in ix's list order
 *             inside every list.  Compatibility as above.  subset_type 0 (SUBSET_TYPE_ID_RANGE): stored id in [a1, a2).  1
 *             (SUBSET_TYPE_ID_MOD): id % a1 == a2 with C's % on int64; a1 <= 0 is refused.  2 (SUBSET_TYPE_ELEMENT_RANGE): walking the lists
 *             l = 0 .. nlist-1 with running sums accu_n = accu_a1 = accu_a2 = 0, a list of n entries gives next_n = accu_n + n,
 *             i1 = next_n * a1 / ntotal - accu_a1, i2 = next_n * a2 / ntotal - accu_a2 (integer divisions); entries [i1, i2) of the list are
 *             copied, then accu_n = next_n, accu_a1 += i1, accu_a2 += i2.  UNVERIFIED: restated from FAISS's InvertedLists::copy_subset_to
 *             from memory, like the file layouts.  What does not depend on memory is tested: consecutive (a1, a2) ranges that tile
 *             [0, ntotal) miss no listed row, and select every listed row exactly once unless a part meets a list whose rounded range is
 *             inverted (i1 > i2: nothing of that list is copied and the neighbouring parts overlap there).  The formula does not exclude
 *             that for lists much smaller than a part (ntotal 7, three rows before a list of one row, cuts 2 | 3 | 4 take its row twice);
 *             a part whose share n (a2 - a1) / ntotal of every non-empty list is at least two entries is safe.  Any other value fails with "subset type not implemented".
 *   out       merging across devices, pre-transform / refine / HNSW / sharded / binary merges, subset types 3 and 4. */
int mvs_index_merge_from(mvs_index *ix, mvs_index *other, int64_t add_id);
int mvs_index_check_compatible_for_merge(const mvs_index *ix, const mvs_index *other);
int mvs_index_ivf_copy_subset_to(const mvs_index *ix, mvs_index *other, int subset_type, int64_t a1, int64_t a2);

/* ---- selector programs: MVS_SEL_PROGRAM -- faiss::IDSelectorRange, IDSelectorArray, IDSelectorAll, IDSelectorNot, IDSelectorAnd,
 * IDSelectorOr and IDSelectorXOr (faiss/impl/IDSelector.h), alone and nested.  The reference glue builds none of them (it constructs
 * IDSelectorBitmap and IDSelectorBatch only, src/faiss_extension.cpp:959,:1008); they are what a database caller wants for WHERE id BETWEEN a
 * AND b, for "exclude these m rows" without a bitmap of n bits, for a cached tenant bitmap combined with a per-query range, and for DELETE
 * ... WHERE id < x.  The membership rules below restate those classes FROM MEMORY: no FAISS source was at hand.  THESE RULES are the
 * contract:
 *   form      sel_kind = MVS_SEL_PROGRAM, sel_data = an array of mvs_sel_node, sel_n = the node count.  The same triple is accepted by
 *             mvs_index_search (and search_and_reconstruct), mvs_index_range_search, mvs_index_remove_ids and by the binary family's search
 *             and range_search.  The nodes and everything they point to are HOST memory owned by the caller for the duration of the call.
 *   evaluation  postfix, per tested id: a leaf (ALL, BITMAP, BATCH, ARRAY, RANGE) pushes its truth value, NOT replaces the top, AND / OR / XOR
 *             pop two and push one.  A well-formed program leaves exactly one value: the id is a member iff it is true.  At most 64 nodes,
 *             and so a stack of at most 64.
 *   leaves    RANGE: id >= imin && id < imax (IDSelectorRange's assume_sorted has no meaning here and is ignored).  ARRAY and BATCH: the
 *             id occurs in the list; duplicates are harmless; n == 0 admits nothing (FAISS's two classes differ only in cost).  BITMAP:
 *             exactly the rule of MVS_SEL_BITMAP -- the id is read as uint64 and bit `id` is tested; beyond the bitmap is not a member, so
 *             NOT(BITMAP) admits negative ids and ids past its end.  ALL: true.  NOT, AND, OR, XOR: the Boolean operation.
 *   tested id whatever the plain selectors test for that kind and call: label_offset + row (Flat, PQ, SQ8), the stored id of an IVF kind,
 *             the external id under IDMap, the vertex id of HNSW, the binary family's row or id_map entry.
 *   errors    a malformed program fails the call with a text naming the node index and the reason ("selector program: node <i>: ..."):
 *             an unknown op, a stack underflow, more than one value left, zero nodes, more than 64 nodes, n < 0, NULL data with n > 0.  The
 *             index is untouched.  MVS_SEL_NONE for remove_ids is still an error, and any other sel_kind is still unknown.
 *   promise   for every kind and every entry point that takes a selector, a call with a program returns bit for bit what the same call
 *             returns with MVS_SEL_BATCH of exactly the admitted ids among the ids in the index: distances, labels, hit order, n_removed and
 *             the resulting store.
 *   lowering  no scan knows programs.  Per call the program is evaluated on the device over the ids the call's scan will test (after staged
 *             rows are flushed, so they are seen) and becomes one of the two plain selectors: nothing admitted -> a batch of no ids; every
 *             admitted id >= 0 and max / 8 + 1 <= the cap -> a bitmap of max / 8 + 1 bytes; else a batch of the admitted ids, sorted on the
 *             device.  The (count, min, max) of the admitted ids are read back once: one stream synchronisation per call, where
 *             MVS_SEL_BATCH sorts on the host.  IVF kinds evaluate remove_ids's program on the host, where their removal plan is made.  A
 *             one-leaf program of BITMAP or of BATCH / ARRAY takes MVS_SEL_BITMAP's / MVS_SEL_BATCH's path unchanged: no evaluation.
 * mvs_index_set_option (and mvs_binary_index_set_option): "sel_bitmap_cap_bytes" = the largest bitmap a program is lowered to (0: automatic,
 * max(1 MiB, 2 bytes per tested id)).  mvs_index_get_stat (mvs_binary_index_get_stat): "sel_lowered" = 0 none | 1 bitmap | 2 batch for the last
 * call of the handle that evaluated a program, "sel_admitted" = the admitted ids it counted (with multiplicity).  A sharded index lowers the
 * program per shard and reports 0 for both. */
#define MVS_SELOP_ALL 1
#define MVS_SELOP_BITMAP 2
#define MVS_SELOP_BATCH 3
#define MVS_SELOP_ARRAY 4
#define MVS_SELOP_RANGE 5
#define MVS_SELOP_NOT 6
#define MVS_SELOP_AND 7
#define MVS_SELOP_OR 8
#define MVS_SELOP_XOR 9
typedef struct mvs_sel_node {
	int32_t op;         /* MVS_SELOP_* */
	int32_t reserved;   /* 0 */
	const void *data;   /* BITMAP: bytes; BATCH / ARRAY: int64 ids; else NULL */
	int64_t n;          /* BITMAP: bytes; BATCH / ARRAY: ids; else 0 */
	int64_t imin, imax; /* RANGE */
} mvs_sel_node;

/* ---- reconstruct: faiss::Index::reconstruct(key, recons), reconstruct_n(i0, ni, recons), reconstruct_batch(n, keys, recons) and
 * search_and_reconstruct(n, x, k, distances, labels, recons, params) -- hand stored vectors back.  The reference glue never calls them; they
 * are what a re-ranker above the library, a recall debugger, or a caller who wants the vectors of the hits together with the hits needs
 * instead of write_index and a parser of its own.  The rules below restate Index::reconstruct*, IndexFlatCodes::reconstruct_n,
 * IndexIVF::reconstruct / reconstruct_n / reconstruct_from_offset with a hash-table DirectMap, IndexIDMap2::reconstruct and
 * IndexRefine::reconstruct FROM MEMORY.  THESE RULES are the contract:
 *   a reconstruction   is the row as the index STORES it, as d f32 values, bit for bit:
 *             Flat, HNSW<M>[,Flat], IVF<n>,Flat, IVF<n>_HNSW<m>,Flat   the f32 row that was added.
 *             PQ<M>                 sub-vector m is codebook entry code[m], a copy.
 *             SQ8, HNSW<M>,SQ8      a[k] + (float)c s[k]: one multiplication and one addition, each rounded on its own (the decode of the
 *                                   "8-bit scalar-quantised indexes" section).
 *             IVF<n>,PQ<M>, IVF<n>,SQ8   the decoded residual first, then ONE f32 addition of the list's centroid per component (the order of
 *                                   reconstruct_from_offset).  No operation is contracted into an fma.
 *             <base>,RFlat          the refine store's f32 row (IndexRefine::reconstruct).
 *   key -> row   kinds without stored ids (Flat, PQ, SQ8, the HNSW kinds, Refine): key - label_offset is the arrival position.  IVF kinds: the
 *             row whose STORED id is the key.  Under IDMap, / IDMap2,: the row whose external id is the key.  Where several rows carry the key
 *             the row added LAST wins, as FAISS's hash-table direct map and IndexIDMap2::rev_map do (both overwrite).
 *             DEPARTURE FROM FAISS: the IVF kinds need no make_direct_map -- the (key, position) table is built on the device on first use
 *             and dropped by add, remove_ids, an image load and a move to another device.
 *             DEPARTURE FROM FAISS: "IDMap," serves reconstruction as "IDMap2," does (FAISS's IndexIDMap refuses); the map is on the device anyway.
 *   errors    a key that names no row: an error whose text holds "key not found" and the key; a kind without ids answers with FAISS's
 *             "Error: 'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed" instead.  A batch reports the FIRST missing key in batch order;
 *             recons is unspecified after an error.  A sharded index and any kind not listed answer with FAISS's base-class text
 *             "reconstruct not implemented for this type of index", whatever n is.  (One rank's part of a per-rank sharded index is an
 *             ordinary index with a label offset: it answers for its own rows.)
 *   reconstruct_n(i0, ni)   kinds without ids: the positions i0 .. i0+ni-1.  Under IDMap: the external keys i0 .. i0+ni-1, each of which
 *             must exist.  A bare IVF kind, as IndexIVF::reconstruct_n: the rows whose stored id lies in the range, written at id - i0; the
 *             rows of absent ids are left untouched.
 *   search_and_reconstruct   distances and labels are exactly what search writes for the same arguments (selectors, nprobe, efSearch,
 *             k_factor); recons[q][j] is the reconstruction of labels[q][j]; for a label of -1 every byte of the row is 0xFF (FAISS's
 *             memset(..., -1, ...)).  The row is found through the LABEL: with duplicate ids the row shown is the last added one, not
 *             necessarily the one matched (carrying the matched position through the emit kernels is out of scope).
 *   edges     n = 0, ni = 0, an empty index and k-padding work.  Rows staged by add() are flushed first.  Nothing in the index changes: a
 *             search before and after gives identical results.
 *   device    the _device variants take device pointers for keys, queries and outputs and order their work on `stream`.
 *             search_and_reconstruct_device never visits the host; reconstruct_batch_device reads one word back after the gather (the first
 *             missing batch index), so it returns once `stream` has passed the call.
 * Statistic recon_pq_lds (mvs_index_get_stat): the handle's last PQ decode read its codebooks from LDS (1: they fit in 128 KB, d <= 128, and
 * the call writes at least as many bytes as it loads) or through L2 (0); -1 before the first. */
int mvs_index_reconstruct(mvs_index *ix, int64_t key, float *recons /* d */);
int mvs_index_reconstruct_n(mvs_index *ix, int64_t i0, int64_t ni, float *recons /* ni*d */);
int mvs_index_reconstruct_batch(mvs_index *ix, int64_t n, const int64_t *keys, float *recons /* n*d */);
int mvs_index_search_and_reconstruct(mvs_index *ix, int64_t n, const float *x, int64_t k, float *distances, int64_t *labels,
                                     float *recons /* n*k*d */, const mvs_search_params *params);
/* device-resident: keys, outputs and queries are device pointers, work is ordered on `stream`, no host visit on the success path */
int mvs_index_reconstruct_batch_device(mvs_index *ix, int64_t n, const int64_t *d_keys, float *d_recons, void *stream);
int mvs_index_search_and_reconstruct_device(mvs_index *ix, int64_t n, const float *d_x, int64_t k, float *d_distances, int64_t *d_labels,
                                            float *d_recons, const mvs_search_params *params, void *stream);

/* faiss::gpu::index_cpu_to_gpu(resources, device, index)  -- src/gpu/gpu.cpp:48.
 * Indexes are already device-native; this migrates the index to `device` (no-op if it is there). */
int mvs_index_to_gpu(mvs_index *ix, int device);
int mvs_index_device(const mvs_index *ix);
/* the same call with FAISS's ownership: returns a NEW index on `device` holding a copy of `src` (the glue replaces
 * entry.index with the result and drops the old object, src/gpu/gpu.cpp:48) */
int mvs_index_clone_to_gpu(mvs_index **out, const mvs_index *src, int device);

/* ---- several devices behind the same surface -------------------------------------------------
 * The reference's hook names ONE device (MoveToGPUFunction, src/gpu/gpu.cpp:34-63 -> index_cpu_to_gpu(res, device,
 * index) :48).  Three ways reach all GPUs of the node WITHOUT touching src/faiss_extension.cpp:
 *   - faiss_to_gpu(name, -1): mvs_index_clone_to_gpu(out, src, -1) returns the index spread over every device of env
 *     MVS_DEVICES ("0,1,...,7"; default: all visible devices);
 *   - env MVS_DEVICES set when faiss_create / faiss_load run: mvs_index_factory / mvs_read_index build it sharded;
 *   - mvs_index_shard_to_gpus: the same conversion in place, for hosts that hold the handle.
 * Flat / IDMap,Flat / IVF<n>,Flat are ROW-SHARDED (IVF: one set of centroids, trained once, on every device; every
 * inverted list split); HNSW is REPLICATED and the queries are split.  Results are identical to the single-device
 * index bit for bit (labels and distances, including inner-product boundary ties): one exchange of the per-shard
 * (value, global row) blocks -- option "shard_exchange" 0 = per-device D2H, 1 = one ncclAllGather over xGMI -- then the
 * host k-way merge.  mvs_index_shard_info returns the shard count (0 = not sharded). */
int mvs_index_shard_to_gpus(mvs_index *ix, const int *devices, int ndev);
int mvs_index_shard_info(const mvs_index *ix, int *devices, int max_devices, int64_t *rows_per_shard,
                         int64_t *last_tie_queries);

/* faiss::write_index / read_index  -- src/faiss_extension.cpp:199,234 */
int mvs_write_index(const mvs_index *ix, const char *filename);
int mvs_read_index(mvs_index **out, const char *filename);

/* ---- binary indexes: faiss::IndexBinary, FAISS's second family -- bit vectors compared by Hamming distance: "BFlat"
 * (faiss::IndexBinaryFlat) alone or under "IDMap," / "IDMap2," (faiss::IndexBinaryIDMap / IndexBinaryIDMap2).  The reference glue never
 * builds one; 1-bit-quantised embeddings, perceptual hashes and LSH sketches are what they hold (a 1024-bit code is 128 bytes where the
 * f32 row is 4 KB).  The family has a door of its own, as in FAISS: a separate opaque mvs_binary_index, index_binary_factory,
 * read_index_binary, write_index_binary; no mvs_index_* function learns about bits.  The rules below restate IndexBinary.h,
 * IndexBinaryFlat.cpp, IndexBinaryIDMap, utils/hamming.cpp and impl/index_write.cpp FROM MEMORY: no FAISS source was at hand.  THESE
 * RULES are the contract.  Distances are integers: every result is exact by construction.
 *   shape     d is a number of BITS; d % 8 != 0 fails with "Error: 'd % 8 == 0' failed".  code_size = d / 8: a vector is code_size bytes.
 *             metric_type reads 1, is_trained reads true, train is a no-op.  Served: 8 <= d <= 2048; beyond: "This index type is not
 *             implemented on the MI355X path yet: <string> with d = <d> (at most 2048 bits)".
 *   strings   "BFlat", "IDMap,BFlat", "IDMap2,BFlat".  DEPARTURE FROM FAISS: its binary factory has no IDMap prefix -- there one wraps
 *             by hand, which the adaptor class faiss::IndexBinaryIDMap does here too.  "BIVF...", "BHNSW...", "BHash...": "This index type
 *             is not implemented on the MI355X path yet: <string>".  Anything else: "could not parse index string <string>".
 *   distance  ham(q, r) = the population count of q XOR r over the code_size bytes, an int32.
 *   search    per query the admitted rows are ordered by the PAIR (ham, internal row number), ascending, and the first k are returned in
 *             that order.  This is FAISS's result SET -- its heap replaces only on a strictly smaller distance, so the earlier row survives
 *             a tie -- and exactly the order of its counting path (use_heap = false).  DEPARTURE FROM FAISS's default heap path: the order
 *             inside a run of equal distances.  Missing slots (k beyond the admitted rows) are distance 2147483647 with label -1.
 *             1 <= k <= 2048: k <= 0 fails with "Error: 'k > 0' failed", k > 2048 with "k = <k> is beyond the largest k ...".  n == 0 is a
 *             no-op; ntotal == 0 pads everything.
 *   labels    the row number on a bare BFlat, id_map[row] under IDMap.  MVS_SEL_BITMAP / MVS_SEL_BATCH of mvs_search_params test that same
 *             id with the membership rules of the remove_ids section: a negative id is not a member, an id beyond the bitmap is not a
 *             member, duplicates in a batch are harmless.  A row that is not a member takes part neither in the result nor in any bound.
 *             nprobe and efSearch are ignored.
 *   range_search   radius is an int; row r is a hit iff ham < radius, strictly.  A query's hits are in ascending internal row order;
 *             distances are stored as float, as faiss::RangeSearchResult does; the result object is mvs_range_result with its refusal of
 *             more than 2^30 hits in one call.
 *   add       the bare index refuses add_with_ids ("add_with_ids not implemented for this type of index"), IDMap refuses add ("add does
 *             not make sense with IndexBinaryIDMap, use add_with_ids").  Small adds are staged in pinned memory and reach the device once
 *             per slot; every reader sees staged rows.  At most 2^31 - 1024 rows.
 *   reset     ntotal = 0; add works again.
 *   reconstruct(key) / reconstruct_n(i0, ni)   code_size bytes per row, bit for bit the bytes added.  Bare: key is the row number; outside
 *             [0, ntotal): "Error: 'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed".  Under IDMap, / IDMap2,: the row whose external id
 *             is the key, the row added LAST where several carry it, "key not found: <key>" where none does; reconstruct_n names the keys
 *             i0 .. i0 + ni - 1, each of which must exist.  DEPARTURE FROM FAISS: "IDMap," serves it as "IDMap2," does.
 *   files     mvs_write_index_binary / mvs_read_index_binary.  "IBxF": fourcc, int32 d, int32 code_size, int64 ntotal, uint8 is_trained,
 *             int32 metric_type, then the codes as a FAISS vector (uint64 count of bytes, the bytes).  "IBMp" ("IBM2" for IDMap2): the same
 *             header, the sub-index's image, id_map as uint64 count + int64s.  The bytes are RESTATED FROM MEMORY and not pinned against a
 *             FAISS build.  Refused with a message naming the offending value: a truncated file, a fourcc that is not a binary index's (a
 *             float index file), a code_size other than d / 8, a byte count other than ntotal x code_size, an id_map of another length.
 *             mvs_read_index refuses a binary file through its unknown-fourcc path.
 *   refusals  out of scope and refused where a call exists: BIVF, BHNSW, BHash; remove_ids, sharding and clone_to_gpu (no entry point);
 *             k > 2048; d > 2048.  The device is the one env MVS_DEVICE names; without a usable GPU every call fails ("no CPU fallback").
 *   hot path  csrc/binary.hip: rows in word-major tiles of 64, lanes hold rows, queries arrive as wave-uniform operands -- one XOR and one
 *             accumulating population count per 32 bits of a pair.  The scan keeps no k-lists: a row goes to a candidate stream iff its
 *             pair (ham, row) is below the query's bound, the exact k-th smallest pair of the rows scanned in earlier GENERATIONS (launches
 *             over geometrically growing row ranges); a finish sorts a query's records by ham << 32 | row.  A stream that overflows is
 *             detected and the generation scanned again with room; results depend on neither option below.
 * mvs_binary_index_set_option: "binary_first_rows" = rows examined before the first bound exists (default 256; at least k are taken),
 * "binary_stream_cap" = entries of the candidate stream's first attempt, and of range_search's hit stream (0: automatic).
 * mvs_binary_index_get_stat: "binary_scan_launches" / "binary_candidates" = scan launches / stream records of the last search,
 * "binary_rescans" = scans repeated because a stream was too small, over the index's life, "binary_add_flushes" = transfers of staged rows
 * to the device, over the index's life, "device_bytes_live" = the process-wide figure mvs_index_get_stat gives under that name. */
#define MVS_BINARY_KIND_FLAT 1  /* faiss::IndexBinaryFlat  */
#define MVS_BINARY_KIND_IDMAP 2 /* faiss::IndexBinaryIDMap */
typedef struct mvs_binary_index mvs_binary_index;
/* faiss::index_binary_factory(d, description); the index lives on the device env MVS_DEVICE names (default 0) */
int mvs_binary_index_factory(mvs_binary_index **out, int d, const char *description);
void mvs_binary_index_free(mvs_binary_index *ix);
/* IndexBinary::d / code_size / ntotal; MVS_BINARY_KIND_* */
int mvs_binary_index_d(const mvs_binary_index *ix);
int mvs_binary_index_code_size(const mvs_binary_index *ix);
int64_t mvs_binary_index_ntotal(const mvs_binary_index *ix);
int mvs_binary_index_kind(const mvs_binary_index *ix);
/* IndexBinaryIDMap::index: a borrowed handle on the wrapped IndexBinaryFlat (labels and selector ids are row numbers; it takes no rows
 * itself), NULL if the index is not an IDMap */
mvs_binary_index *mvs_binary_index_idmap_sub(mvs_binary_index *ix);
/* IndexBinary::add(n, x) / add_with_ids(n, x, ids): x is n * code_size bytes */
int mvs_binary_index_add(mvs_binary_index *ix, int64_t n, const uint8_t *x);
int mvs_binary_index_add_with_ids(mvs_binary_index *ix, int64_t n, const uint8_t *x, const int64_t *ids);
/* IndexBinary::search(n, x, k, distances, labels, params) */
int mvs_binary_index_search(mvs_binary_index *ix, int64_t n, const uint8_t *x, int64_t k, int32_t *distances, int64_t *labels,
                            const mvs_search_params *params);
/* IndexBinary::range_search(n, x, radius, result, params) */
int mvs_binary_index_range_search(mvs_binary_index *ix, int64_t n, const uint8_t *x, int radius, const mvs_search_params *params,
                                  mvs_range_result **out);
/* IndexBinary::reset / reconstruct / reconstruct_n: code_size bytes per row */
int mvs_binary_index_reset(mvs_binary_index *ix);
int mvs_binary_index_reconstruct(mvs_binary_index *ix, int64_t key, uint8_t *recons /* code_size */);
int mvs_binary_index_reconstruct_n(mvs_binary_index *ix, int64_t i0, int64_t ni, uint8_t *recons /* ni*code_size */);
/* device-resident variants: device pointers, ordered after and before `stream` (d_ids NULL on a bare index, given under IDMap) */
int mvs_binary_index_add_device(mvs_binary_index *ix, int64_t n, const uint8_t *d_x, const int64_t *d_ids, void *stream);
int mvs_binary_index_search_device(mvs_binary_index *ix, int64_t n, const uint8_t *d_x, int64_t k, int32_t *d_distances, int64_t *d_labels,
                                   const mvs_search_params *params, void *stream);
int mvs_binary_index_set_option(mvs_binary_index *ix, const char *key, int64_t value);
int mvs_binary_index_get_stat(mvs_binary_index *ix, const char *name, int64_t *value);
/* faiss::write_index_binary / read_index_binary */
int mvs_write_index_binary(mvs_binary_index *ix, const char *filename);
int mvs_read_index_binary(mvs_binary_index **out, const char *filename);

/* ---- device-resident variants (same semantics, inputs/outputs already in HBM) --------------------
 * Used by bench.py (the metric is quoted with inputs resident in HBM) and by the multi-GPU host,
 * which hands the per-shard (distance,label) blocks to RCCL without a host round trip.
 * `stream` is a hipStream_t used exactly as given (NULL = HIP's null stream, which is PyTorch's default
 * stream); the call only enqueues work and is ordered after/before the index's own host-API stream with
 * events, so host-API and device-API calls may be mixed freely. */
int mvs_index_add_device(mvs_index *ix, int64_t n, const float *d_x, const int64_t *d_ids, void *stream);
int mvs_index_search_device(mvs_index *ix, int64_t n, const float *d_x, int64_t k, float *d_distances,
                            int64_t *d_labels, const mvs_search_params *params, void *stream);
/* label offset added to implicit (non-IDMap) labels: row-sharded multi-GPU search returns GLOBAL ids */
int mvs_index_set_label_offset(mvs_index *ix, int64_t offset);

/* k-way merge of per-shard results [nshard][n][k] (global labels) with the FAISS ordering rule.
 * Host arrays.  This is the "host k-way merge" that follows the RCCL all-gather. */
int mvs_merge_shards(int metric, int64_t n, int64_t k, int nshard, const float *D, const int64_t *I, float *D_out,
                     int64_t *I_out);

/* The same merge ON THE DEVICE, straight from the gathered records: d_records = [nshard][n][kk][2] int64 {value bits in the
 * low word, global label} as the all-gather delivers them (pyhost/sharded.py pack_records); keeps the kout <= kk best per
 * query.  raw = 1: the pure order (what step 1 of the tie protocol below needs); raw = 0: FAISS's print order.  With 8
 * GPUs the per-rank search of the headline is ~3 ms and a host merge of 8 x 10k x 10 candidates costs more than that. */
int mvs_merge_records_device(int metric, int64_t n, int kk, int kout, int nshard, const int64_t *d_records, int raw,
                             float *d_D_out, int64_t *d_I_out, void *stream);

/* ---- inner-product boundary ties across PROCESSES (one rank per GPU, pyhost/sharded.py under torchrun) ----------
 * FAISS's CMin heap keeps an arrival-order dependent subset of the rows tied at the k-th score.  A row
 * shard therefore hands over its k+1 best in the PURE order (option "ip_exact_ties" = 0, search with k+1):
 *   1. gather, mvs_merge_shards_raw -> merged top-(k+1), pure order;
 *   2. queries whose k-th and (k+1)-th scores are bit-equal: every rank reports, per such query, its k smallest GLOBAL
 *      rows with score >= T (mvs_index_tie_candidates_device; T = the k-th score), gather, keep the k smallest;
 *   3. mvs_finish_ip_ties writes FAISS's print order for all queries and the heap's outcome for the flagged ones.
 * (A ShardedIndex does the same inside the library.) */
int mvs_merge_shards_raw(int metric, int64_t n, int64_t kk, int nshard, const float *D, const int64_t *I, float *D_out,
                         int64_t *I_out);
int mvs_index_tie_candidates_device(mvs_index *ix, int64_t nf, const float *d_xf, const float *d_T, int64_t k,
                                    int64_t *d_rows_out, const mvs_search_params *params, void *stream);
int mvs_finish_ip_ties(int64_t n, int64_t k, int64_t kk, const float *raw_D, const int64_t *raw_I, int64_t nf,
                       const int64_t *flagged, const int64_t *first_rows, float *D_out, int64_t *I_out);

/* ---- IVF exact distance ties across PROCESSES (round 5; DESIGN.md 3.5 "row-sharded IVF") ----------------------------------
 * FAISS's IVFFlatScanner feeds a heap in ARRIVAL order -- probe rank of the list, then position in the list
 * (IndexIVF::search_preassigned behind /root/reference/src/faiss_extension.cpp:631) -- so which rows tied at the k-th value
 * survive depends on arrival order.  A row shard hands over its k + 1 best in the PURE order (option "ivf_exact_ties" = 0,
 * search with k + 1, stored ids = global rows); for a query whose merged k-th and (k + 1)-th values are bit-equal every
 * rank reports its first k rows NOT WORSE than T in arrival order -- value, stored id, probe rank of the list (-1 padded) --
 * and the merge rank takes the first k of the union by (probe rank, id) = A_k and applies the closed form of csrc/ivf_ties.hip
 * (pyhost/sharded.py merge_ivf_exact; the in-library ShardedIndex does the same in resolve_ties_ivf).
 * d_flag = {nf, query numbers ...} on the device; d_x = the WHOLE batch of the search that has just run on this index (its coarse
 * assignment is reused: the call must follow that search directly -- checked: another d_x, more flagged queries than the batch held or
 * a query number outside it is an error); d_T [nf]; outputs [nf][k].  mvs_index_get_stat "ivf_ids_ascending" = 1 while every id added
 * so far exceeded all before it -- the cross-process merge's arrival order (probe rank, id) is FAISS's only then. */
int mvs_index_ivf_tie_emit_device(mvs_index *ix, int64_t nf, const int *d_flag, const float *d_x, const float *d_T, int64_t k,
                                  float *d_v_out, int64_t *d_id_out, int *d_rank_out, const mvs_search_params *params,
                                  void *stream);

/* ---- synthetic data (counter-based, identical on host oracle and device) and diagnostics -------- */
int mvs_synth_uniform_device(float *d_out, int64_t n_rows, int d, uint64_t seed, int64_t row0, void *stream);
int mvs_synth_clustered_device(float *d_out, int64_t n_rows, int d, uint64_t seed, int64_t row0, int n_centers,
                               float sigma, void *stream);
/* name + launch geometry + algorithmic flops/bytes of the dominant kernel of the last search on this
 * index (bench.py's roofline object); returns 0 and fills the fields */
typedef struct mvs_kernel_info {
	char name[64];
	double flops;       /* algorithmic flops of the launch            */
	double bytes;       /* algorithmic HBM bytes of the launch        */
	double last_ms;     /* HIP-event duration of that launch, if timed */
	int32_t grid, block, lds_bytes, nsplit;
} mvs_kernel_info;
/* Diagnostics (no counterpart in the reference): ntiles independent v_mfma_f32_16x16x32_bf16 instructions, D = A B + C, on host
 * buffers -- A [ntiles][16 rows][32 k] and Bt [ntiles][16 columns][32 k] as bf16 bit patterns, C / D [ntiles][16][16] f32.  The
 * coarse filters' error bound models this instruction's internal accumulation; tests/test_mfma_model_gpu.py measures it. */
int mvs_debug_mfma_bf16_16x16x32(const uint16_t *A, const uint16_t *Bt, const float *C, float *D, int64_t ntiles);
int mvs_index_last_kernel_info(const mvs_index *ix, mvs_kernel_info *out);
/* when enabled, the dominant kernel of every search is bracketed by HIP events on its stream */
int mvs_index_set_kernel_timing(mvs_index *ix, int enabled);
/* number of timed launches so far and the sum of their HIP-event durations */
int mvs_index_kernel_time_stats(mvs_index *ix, int *count, double *total_ms);
/* implementation knobs (never needed by the reference glue): "force_direct" = 0/1 */
int mvs_index_set_option(mvs_index *ix, const char *key, int64_t value);
/* bf16x3 prefilter of the Flat BLAS-branch search (csrc/flat_bf16.hip; results are those of the exact f32 kernel): queries
 * it served so far, how many of them could not be proven and were re-run on the exact kernel, the largest observed
 * |approx - exact| / (||x|| ||y||) among re-scored candidates and the bound c(d) the proof uses.  An IVF<n>,Flat index reports the
 * first two figures for its own filters (re-run = on the scanner kernel), the other two as 0 */
int mvs_index_prefilter_stats(mvs_index *ix, int64_t *queries, int64_t *fallback_queries, float *max_rel_err,
                              float *err_bound);
/* bf16 coarse filter of the same search (csrc/flat_collect.hip; option prefilter = 2): queries it served, candidates it
 * re-scored exactly for them, batches whose candidate stream overflowed (served by the bf16x3 path instead) */
int mvs_index_collect_stats(mvs_index *ix, int64_t *queries, int64_t *candidates, int64_t *overflows);
/* IVF, diagnostics: the (query, probed list) pairs of the index's last coarse-filter search (nq x nprobe) and how many of them were
 * scanned.  IndexIVF::search (faiss/IndexIVF.cpp search_preassigned, reached from src/faiss_extension.cpp:631) scans every probed
 * list; this path leaves out the lists that PROVABLY hold none of a query's k nearest rows (triangle inequality on the coarse
 * distance and the list's radius, option ivf_probe_prune, L2 without an IDSelector) -- labels and distances are unchanged.
 * forced_drains: how often a scan wavefront of the last search had to empty its LDS hit queue in the middle of a tile.
 * admitted: candidates the scan of the last search admitted under its running bounds; mvs_index_collect_stats counts those that
 * also passed the bound the scan ended with and were re-scored exactly (option ivf_cl_refilter). */
int mvs_index_ivf_probe_stats(mvs_index *ix, int64_t *pairs, int64_t *pairs_scanned, int64_t *forced_drains, int64_t *admitted);
/* Flat L2 index, diagnostics of its shadow clustering (rows that cluster are answered through an internal IVF index of the same rows
 * with a per-query exactness proof, csrc/index.hip FlatIndex::shadow_search -- results are those of faiss::IndexFlat::search,
 * src/faiss_extension.cpp:631).  stats[8] = {state (0 not wanted, 1 in use, -1 given up on this data), rows the shadow holds (-1: none),
 * queries answered through it, of those re-run on the Flat kernels (unproven), builds (k-means), extensions (rows appended after
 * add()), device bytes the shadow holds, its nlist}; build_seconds = time spent building / extending it inside search calls. */
int mvs_index_shadow_stats(mvs_index *ix, int64_t *stats, double *build_seconds);
/* diagnostics by name (tests, bench): "coarse_bf16_queries" = queries of an IVF index whose coarse quantisation (IndexIVF::search ->
 * quantizer->search, src/faiss_extension.cpp:631) ran as a bf16 filter + exact re-scoring (csrc/coarse_bf16.hip);
 * "coarse_bf16_exhaustive" = of those, queries that were computed against every centroid (list overflow / no finite bound);
 * "coarse_bf16_candidates" = centroids re-scored exactly in the last such call, summed over its queries; "flat_outlier_rows" = rows of a
 * Flat index kept out of its bf16 coarse-filter store because of their norm (they join every query's candidates: csrc/flat_collect.hip);
 * "hnsw_build_distances" / "hnsw_build_shortcuts" = distance evaluations of an HNSW index's builds so far / add_link calls that took the
 * full-list short cut instead of HNSW::shrink_neighbor_list's pairwise pass (csrc/hnsw.hip; IndexHNSW::add, src/faiss_extension.cpp:510);
 * "device_bytes_live" = bytes of device memory the PROCESS holds through the owning types of csrc/dev_mem.h, whatever handle asks: the
 * rows, codes, graphs, parameters and workspaces of every index kind, the binary ones included (mvs_binary_index_get_stat answers the
 * same name with the same number) */
int mvs_index_get_stat(mvs_index *ix, const char *name, int64_t *value);
/* named ranges for rocprofv3 --marker-trace (roctx; bound at run time, only under a profiler or with MVS_ROCTX=1): the library
 * marks its own stages (row staging, Flat / IVF search, shard search, exchange, merge); a host that merges shard results itself
 * (pyhost/sharded.py: the exchange of src/gpu/gpu.cpp:48's multi-GPU layout) brackets its stages with these */
int mvs_trace_push(const char *name);
int mvs_trace_pop(void);
int mvs_device_count(void);
const char *mvs_version(void);

#ifdef __cplusplus
}
#endif
#endif
