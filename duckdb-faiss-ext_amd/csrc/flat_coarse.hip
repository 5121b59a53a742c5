// csrc/flat_coarse.hip -- host side of the Flat coarse filter: the derived row stores, one pass of the filter as a driver over named
// stages (FlatIndex::collect_candidates), and the search that wraps it (FlatIndex::search_prefilter).  Host code only: the kernels are
// in csrc/flat_collect*.hip and csrc/ivf_collect.hip.
//
// A search flows   FlatSearchRequest -> search_prefilter_pass -> CollectRequest -> collect_candidates { plan -> stores -> workspaces -> query preparation and
// bounds -> scan with overflow handling -> one of three finishes } -> CollectResult -> emission, report, tie pass, re-run of the
// unproven queries.  What a pass needs and leaves travels in those two structs (csrc/index.h); the index keeps only what outlives a
// search (see "what the coarse filter keeps BETWEEN searches" there).
#include "flat_collect.h"
#include "collect_launch.h"
#include "index.h"

#include <algorithm>
#include <cstring>

namespace mvs {

// the same as ensure_bf16_rows for the coarse filter's store: rows as bf16 only (csrc/flat_collect.hip)
void FlatIndex::ensure_h1_rows(hipStream_t st) {
	if (h1.n == ntotal && vecs_h1())
		return;
	const int dp1 = collect_store_dims(d); // row pitch of the bf16 store: 128 up to d = 128, else 256 / 384 / 512
	ensure_max_norm_bits(st);
	if (!mu_h1) { // the centre is fixed at the first build (any vector is valid; rows added later only fit it less well)
		mu_h1 = DevBlock<float>((size_t)std::max(geom.dp, 1024));
		const int64_t nm = std::min<int64_t>(ntotal, (int64_t)1 << 20);
		launch_collect_mean(geom, vecs(), nm, mu_h1.get(), st);
		// ... and so is the outlier threshold tau = 64 x the mean ||y - mu||^2 of those rows (csrc/flat_collect.hip "outlier rows").  Only
		// stores large enough for the coarse filter to matter: an IVF quantiser's centroids, which csrc/coarse_bf16.hip searches through
		// this store too, are never taken out of it.
		const unsigned inf_bits = 0x7f800000u;
		MVS_HIP(hipMemcpyAsync(d_max_norm_bits.get() + CL_NORM_TAU, &inf_bits, sizeof inf_bits, hipMemcpyHostToDevice, st));
		if (ntotal >= 262144 && outlier_rows) {
			d_outl = DevBlock<int>(1 + CL_OUTL_CAP);
			MVS_HIP(hipMemsetAsync(d_outl.get(), 0, d_outl.cap, st));
			launch_collect_outlier_threshold(norms(), nm, mu_h1.get(), geom.d, d_max_norm_bits.get(), st);
		}
		MVS_HIP(hipStreamSynchronize(st)); // (inf_bits is a stack variable)
	}
	if (ntotal > h1.cap || !vecs_h1())
		h1.grow(std::max<int64_t>(cap, ntotal), st);
	if (dp1 > 128) // csrc/flat_collect_wide.hip
		launch_rows_to_bf16_wide(metric, vecs(), geom.dp, geom.pair_interleaved ? 1 : 0, d, dp1, h1.n, ntotal - h1.n, mu_h1.get(), vecs_h1(),
		                         beta_h1(), norms(), d_max_norm_bits.get(), st, d_outl.get());
	else {
		CollectStoreRows r;
		r.metric = metric, r.vecs = vecs(), r.row0 = h1.n, r.nrows = ntotal - h1.n, r.mu = mu_h1.get();
		r.bf = vecs_h1(), r.beta = beta_h1(), r.norms = norms(), r.max_norm_bits = d_max_norm_bits.get(), r.outl = d_outl.get();
		launch_rows_to_bf16_hi(geom, r, st);
	}
	h1.n = ntotal;
	if (d_outl) { // (one 4-byte read per conversion: the scans' launch code needs to know whether there is anything to append)
		int cnt = 0;
		MVS_HIP(hipMemcpyAsync(&cnt, d_outl.get(), sizeof cnt, hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		h1_outliers = std::min(cnt, CL_OUTL_CAP);
		outl_total = cnt;
	}
}

void FlatIndex::drop_i8() {
	i8.drop();
	d_i8_bits.release();
}

static float word_as_float(const unsigned *words, int i) {
	float v;
	memcpy(&v, words + i, sizeof v);
	return v;
}

// The int8 store (csrc/flat_collect.hip "int8 store") behind the bf16 one, for stores of >= 262 144 rows of d <= 128.  At
// the first build: sy = the power of two with max |y'_i| <= 1.01 x 128 sy (the ends clamp by a step or two), unit = alpha sy^2, the
// query scale sa = alpha sy (queries distributed like the rows: alpha max |x'_i| <= 128 sa); then the format is chosen ONCE: int8 when the
// predicted E_i8 / E_bf16 of a query at the store's largest norm is <= 4 -- E_bf16 ~ 2 alpha ||y'|| ||y' - bf(y')||_max (query residual ~
// row residual), E_i8 ~ ||y'|| (sa sqrt(d / 12) + alpha ||y' - sy Y||_max) -- and every s_int stays below 2^24 (max |beta_int| + d 2^14).
// Rows added later are quantised with the same scales (clamping is in the residual maximum); a range that no longer holds drops the store.
bool FlatIndex::ensure_i8_rows(hipStream_t st) {
	if (!cl_i8 || i8_state < 0 || collect_store_dims(d) != 128)
		return false;
	if (i8_state == 0 && ntotal < 262144) // (the threshold of the outlier rule; an IVF quantiser's centroids never get here)
		return false;
	if (i8_state == 1 && i8.n == ntotal && vecs_i8())
		return true;
	const double alpha = metric == METRIC_L2 ? 2.0 : 1.0;
	if (!d_i8_bits) {
		d_i8_bits = DevBlock<unsigned>(4);
		MVS_HIP(hipMemsetAsync(d_i8_bits.get(), 0, 16, st));
	}
	CollectI8Rows rows;
	rows.vecs = vecs(), rows.mu = mu_h1.get(), rows.beta = beta_h1(), rows.bits = d_i8_bits.get();
	if (i8_state == 0) {
		rows.range = true, rows.row0 = 0, rows.nrows = ntotal;
		launch_rows_to_i8(geom, rows, st);
		unsigned b[4];
		MVS_HIP(hipMemcpyAsync(b, d_i8_bits.get(), 16, hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		const float amax = word_as_float(b, CL_I8_ABS_MAX);
		if (!(amax > 0.f && amax < 1e30f)) {
			i8_state = -1;
			drop_i8();
			return false;
		}
		// (1 % over 128 sy is let clamp: a mean a hair off the middle of the data's range must not cost a whole bit of resolution)
		i8_sy = ldexpf(1.0f, (int)std::ceil(std::log2((double)amax / (128.0 * 1.01))));
		i8_unit = (float)(alpha * (double)i8_sy * (double)i8_sy);
	}
	if (ntotal > i8.cap || !vecs_i8())
		i8.grow(std::max<int64_t>(cap, ntotal), st);
	rows.range = false, rows.row0 = i8.n, rows.nrows = ntotal - i8.n;
	rows.sy = i8_sy, rows.unit = i8_unit, rows.i8 = vecs_i8(), rows.beta_i = beta_i8();
	launch_rows_to_i8(geom, rows, st);
	i8.n = ntotal;
	unsigned b[4], mb[16];
	MVS_HIP(hipMemcpyAsync(b, d_i8_bits.get(), 16, hipMemcpyDeviceToHost, st));
	MVS_HIP(hipMemcpyAsync(mb, d_max_norm_bits.get(), 64, hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	const float res_i8 = word_as_float(b, CL_I8_RESIDUAL), bmax = word_as_float(b, CL_I8_BETA_MAX);
	const float res_bf = word_as_float(mb, CL_NORM_RESIDUAL);
	const bool range_ok = bmax < (float)((1 << 23) - (int64_t)d * 16384); // (NaN / inf: false)
	bool ok = range_ok && res_i8 < 1e30f;
	if (ok && i8_state == 0) {
		const double sa = alpha * i8_sy;
		const double e_i8 = sa * std::sqrt((double)d / 12.0) + alpha * std::sqrt((double)res_i8);
		const double e_bf = 2.0 * alpha * std::sqrt((double)res_bf);
		ok = e_i8 <= 4.0 * e_bf;
	}
	if (!ok) {
		i8_state = -1;
		drop_i8();
		return false;
	}
	i8_state = 1;
	return true;
}

// ---- one pass of the coarse filter ------------------------------------------------------------------------------------------------------

// The shape of a pass, from the request, the index's dimensions and options and what earlier searches learnt: no launch, no allocation
struct CollectPlan {
	bool ok = true; // false: big lists whose row ranges are too short to mean anything (the exact kernels)
	int kf = 0;     // the request's, or kk where it gives none
	int dp1 = 0;    // row pitch of the bf16 store
	int stride = 0; // class slots per query
	bool has_sel = false;
	bool wide = false; // csrc/flat_collect_wide.hip: no one-wavefront-per-segment path
	bool few = false;  // small batch: the one-wavefront-per-segment scan of csrc/ivf_collect.hip
	// lists beyond 128 entries (round 6): the bounds come from a pass of their own over bk_ranges row ranges of bk_rows rows, the scan runs
	// against them frozen, the selection is a segmented sort -- csrc/flat_collect.hip "lists beyond 128 entries"
	bool bigk = false;
	bool bk_seed = false; // ... d <= 128: the ranges are row splits of the register pre-pass kernel
	int bk_ranges = 0;
	int64_t bk_rows = 0;
	int64_t cap_entries = 0; // the candidate stream to start with
	bool fb = false;  // the bucketed finish (see cl_fbucket in csrc/index.h)
	bool wrf = false; // filter-then-sort: the wide big kernel's stream is compacted with the final-bound filter in front of the sort
};

// What the stages of a pass hand to one another
struct CollectWork {
	// what the scan, its pre-passes and the big lists' pass A are launched with (csrc/collect_launch.h): collect_candidates sets the
	// store (i8_unit > 0: the int8 one; the kernels take bytes, see CollectArgs::i8_unit) and the IDSelector's row mask, collect_prepare the rest
	CollectPass pass;
	CollectCtl *ctl = nullptr; // the control block (ws_seg) ...
	int *seg = nullptr;        // ... and the per-query table behind its header
	// collect_workspaces
	int64_t cap_entries = 0;
	unsigned long long *stream = nullptr, *sorted = nullptr; // the two halves of ws_stream
	float *stream_s = nullptr, *fb_thr = nullptr;            // ws_fbk: the coarse value of every entry, the final bound per query
	unsigned *fb_rows = nullptr;                             // ws_fbr: row buckets, key buckets, scatter units,
	unsigned long long *fb_keys = nullptr, *fb_units = nullptr;
	int *fb_kept = nullptr; // per-workgroup survivor counts of the scatter kernel (their sum -> CollectCtl::kept)
	// the scan
	bool defer = false; // the request's defer_count, until something needs the count on the host
	int64_t ncand = 0;  // entries the scan produced (synchronous count mode)
	int grid = 0, nsplit = 0, lds = 0;
	int64_t items = 0; // the plan of the d <= 128 scan: ranges (nsplit) x query blocks
};

static size_t up256(size_t bytes) {
	return (bytes + 255) & ~(size_t)255;
}
static CandStream collect_stream(const CollectWork &w) {
	CandStream s;
	s.entries = w.stream, s.values = w.stream_s, s.count = &w.ctl->count, s.cap = w.cap_entries;
	return s;
}

CollectPlan FlatIndex::collect_plan(const CollectRequest &rq) const {
	CollectPlan pl;
	const int64_t nq = rq.nq;
	const int kk = rq.kk, kf = (rq.kf <= 0 || rq.kf > kk) ? kk : rq.kf;
	pl.kf = kf;
	pl.has_sel = rq.params && rq.params->sel_kind != MVS_SEL_NONE;
	pl.dp1 = collect_store_dims(d);
	pl.stride = collect_slot_stride(kf, pl.dp1, false); // (the bf16 store's; collect_candidates sets the pass's own once the store is chosen)
	pl.wide = pl.dp1 > 128;
	pl.few = !pl.wide && nq <= 128 && kf <= 16 && ntotal < ((int64_t)1 << 31); // (one work item; at 256 queries: 1.92 vs 1.55 ms)
	pl.bigk = kf > 128;
	// (big lists: pass A looks at a quarter of the rows -- any rows give a valid bound, fewer rows a lower one and ~ntotal / rows times k
	// candidates -- unless the candidates of a large batch would not fit: then at all of them)
	// (d <= 128: the ranges are row splits of the register pre-pass kernel, 16 class maxima each, ceil(k / ranges) <= 8 of them decide; the
	// wide stores: 128 class slots per range through the scan kernel's bound-estimation instances, <= 64 decide)
	pl.bk_seed = pl.bigk && !pl.wide;
	constexpr int bk_per = 8; // (rows of a split that decide its bound: the bk_per-th best of its 16 class maxima)
	pl.bk_ranges = pl.bigk ? (pl.bk_seed ? (kf + bk_per - 1) / bk_per : (kf + 63) / 64) : 0;
	if (pl.bk_seed) { // (a small batch has few query blocks: more, shorter splits -- up to four times as many -- fill the device; the bound loosens a little)
		const int nqb = (int)((nq + 511) / 512);
		if (nqb * pl.bk_ranges < 256 && pl.bk_ranges < 64) // (k = 200 at 32 queries: 3.5 -> 2.3 ms; k = 1000 has splits enough and only loses tightness)
			pl.bk_ranges = std::max(pl.bk_ranges, std::min(256 / nqb, 4 * pl.bk_ranges));
	}
	if (pl.bigk) {
		// (a large batch pays the matrix pipe for pass A and the rare path, the gather and the sort for every candidate: all rows = a
		// tighter bound = a third of the candidates; a small batch pays bandwidth: a quarter of the rows)
		// (measured, N = 10 M, profiles/r6_big_k.txt: k = 1000 at 2 048 / 10 000 queries 15.2 / 70 ms on a quarter, 11.2 / 48 on all rows; k = 200: 8.3 / 31 against 13 / 36)
		const bool whole = (nq >= 512 && kf >= 512) || (double)nq * kf * 16.0 > (double)((int64_t)1 << 28);
		const int64_t want = whole ? ntotal : std::max<int64_t>(ntotal / 4, (int64_t)pl.bk_ranges * (pl.bk_seed ? 2048 : 16384));
		pl.bk_rows = std::min<int64_t>(std::max<int64_t>(want / pl.bk_ranges, pl.bk_seed ? 1024 : 4096), ntotal / pl.bk_ranges) / 64 * 64;
		if (ntotal / std::max(pl.bk_ranges, 1) < 192 || pl.bk_rows < 64) {
			pl.ok = false; // (ranges too short to mean anything: the exact kernels)
			return pl;
		}
	}
	// candidate stream: 4096 entries per query to start with (option cl_stream_cap; at least 2^20), or what the last overflow
	// showed this index's data to need (cl_cap_hint, up to 16384 per query: clustered rows with large norms admit thousands)
	pl.cap_entries = cl_stream_cap_per_query > 0 ? std::max<int64_t>(nq * cl_stream_cap_per_query, 1024)
	                                             : std::max<int64_t>(nq * std::max<int64_t>(4096, cl_cap_hint), (int64_t)1 << 20);
	if (pl.bigk && cl_stream_cap_per_query <= 0) // (~ k ntotal / (rows of pass A) candidates per query, times the slack of a class bound)
		pl.cap_entries = std::min<int64_t>(((int64_t)1 << 31) - 4096,
		                                   std::max<int64_t>(pl.cap_entries, nq * std::min<int64_t>(ntotal, 4 * (int64_t)kf * ntotal / std::max<int64_t>(pl.bk_rows * pl.bk_ranges, 1))));
	// the bucketed finish: the common d = 128 shape; round 6: inner product too -- faiss_create's default metric
	// (src/faiss_extension.cpp:105) gets the headline's pipeline, the select kernel prints FAISS's CMin-heap order and the tie flags
	pl.fb = !pl.bigk && cl_fbucket && !cl_fbucket_off && rq.D && (metric == METRIC_L2 || metric == METRIC_IP) && !pl.wide && !pl.few && d == 128 &&
	        geom.dp == 128 && kk <= 64 && nq * (int64_t)cl_fpitch < ((int64_t)1 << 31);
	// (round 5) the 512 < d <= 1536 stores: the big kernel keeps every candidate's coarse value too; the final-bound filter then compacts
	// the stream in front of the sort (a candidate costs 3-6 KB of f32 row there)
	pl.wrf = !pl.fb && !pl.bigk && pl.wide && !strcmp(collect_wide_kernel_name(pl.dp1), "flat_bf16_big_kernel");
	return pl;
}

// The candidate stream (ws_stream), the per-entry values and final bounds (ws_fbk) and the buckets (ws_fbr) for w.cap_entries and
// cl_fpitch; called again after every change of either.  A DevBuf keeps nothing when it grows, so the scan's per-entry values and the
// buckets live in two buffers and each buffer is sized by what IT depends on alone: a larger pitch grows ws_fbr and must not lose the
// values (ws_fbk) or the stream.
void FlatIndex::collect_workspaces(const CollectPlan &pl, int64_t nq, CollectWork &w) {
	const size_t half = up256((size_t)w.cap_entries * 8);
	constexpr size_t pad = 256; // (front of ws_stream: where the counters sat before the control block held them)
	ws_stream.reserve(pad + 2 * half);
	w.stream = (unsigned long long *)((char *)ws_stream.p + pad);
	w.sorted = (unsigned long long *)((char *)ws_stream.p + pad + half);
	if (!pl.fb && !pl.wrf)
		return;
	const size_t sb = up256((size_t)w.cap_entries * 4), tb = up256((size_t)nq * 4);
	ws_fbk.reserve(sb + tb + 256);
	w.stream_s = (float *)ws_fbk.p;
	w.fb_thr = (float *)((char *)ws_fbk.p + sb);
	if (!pl.fb)
		return;
	const size_t rb = up256((size_t)nq * cl_fpitch * 4), kb = (size_t)nq * cl_fpitch * 8;
	const size_t unb = up256(ivf_bucket_units_bytes(w.cap_entries));
	ws_fbr.reserve(rb + kb + unb + (size_t)ivf_bucket_scatter_blocks(w.cap_entries) * 4 + 256);
	w.fb_rows = (unsigned *)ws_fbr.p;
	w.fb_keys = (unsigned long long *)((char *)ws_fbr.p + rb);
	w.fb_units = (unsigned long long *)((char *)ws_fbr.p + rb + kb);
	w.fb_kept = (int *)((char *)ws_fbr.p + rb + kb + unb);
}

// Query fragments, ||x||^2, 2E per query, neutral class slots, the zeroed control block; then the bounds the scan starts from
void FlatIndex::collect_prepare(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w) {
	const int64_t nq = rq.nq;
	hipStream_t st = rq.st;
	ws_qn.reserve((size_t)nq * sizeof(float));
	ws_e2.reserve((size_t)((nq + 255) / 256 * 256) * sizeof(float));
	ws_gthr.reserve((size_t)nq * pl.stride * sizeof(unsigned) * (pl.bigk && !pl.bk_seed ? pl.bk_ranges : 1) + 64);
	if (pl.bk_seed)
		ws_seed.reserve((size_t)pl.bk_ranges * (size_t)nq * 16 * sizeof(float));
	ws_seg.reserve(sizeof(CollectCtl) + (size_t)2 * nq * sizeof(int));
	w.ctl = (CollectCtl *)ws_seg.p;
	w.seg = collect_ctl_table(ws_seg.p);
	// Round 5 (d <= 128 store): fragments, ||x||^2, bounds, neutral class slots and the zeroed control block in ONE launch
	// (csrc/flat_collect.hip collect_query_prep_kernel) instead of four kernels and a memset
	// (the wide stores: separate packing, norm and bound kernels)
	ws_pbnd.reserve(collect_bound_table_bytes(nq)); // (the d <= 128 scan's bound table, and behind it the cursors of its item queues)
	CollectQueryPrep qp;
	qp.metric = metric, qp.x = rq.d_x, qp.nq = nq, qp.d = d, qp.mu = mu_h1.get(), qp.max_norm_bits = d_max_norm_bits.get();
	qp.qn = (float *)ws_qn.p, qp.e2 = (float *)ws_e2.p, qp.fail = {rq.fail_cnt, rq.fail_q};
	if (!pl.wide) {
		ws_pfq.reserve(collect_qfrag_bytes(geom, nq));
		qp.qf = ws_pfq.p;
		qp.gslot = (unsigned *)ws_gthr.p, qp.stride = pl.stride, qp.ctl_hdr = (int *)w.ctl, qp.ctl_seg = w.seg;
		qp.i8_bits = d_i8_bits.get(), qp.i8_unit = w.pass.i8_unit;
		qp.i8_sa = w.pass.i8_unit > 0.f ? (float)(i8_sy * (metric == METRIC_L2 ? 2.0f : 1.0f)) : 0.f;
		qp.cursors = collect_cursors((float *)ws_pbnd.p, nq);
		launch_collect_query_prep(qp, st);
	} else {
		ws_pfq.reserve(collect_qfrag_bytes_ex(pl.dp1, collect_wide_qblock(pl.dp1), nq));
		qp.qf = ws_pfq.p;
		launch_collect_pack_queries_ex(qp, pl.dp1, collect_wide_qblock(pl.dp1), st);
		if (metric == METRIC_L2) // (inner product re-scores without them)
			launch_query_norms(rq.d_x, nq, d, (float *)ws_qn.p, st);
		// (the bounds kernel writes NaN into the slots behind the last query itself)
		launch_collect_bounds(qp, st);
	}
	w.cap_entries = pl.cap_entries;
	collect_workspaces(pl, nq, w);
	// one zeroed control block {stream count | per-query segments} (round 4: one memset instead of three per search)
	if (pl.wide)
		MVS_HIP(hipMemsetAsync(ws_seg.p, 0, sizeof(CollectCtl) + (size_t)2 * nq * sizeof(int), st));
	if (!pl.wide)
		ws_seed.reserve(collect_seed_stage_bytes(nq, pl.stride));
	CollectPass &p = w.pass;
	p.g = geom, p.metric = metric, p.qf = ws_pfq.p, p.n = ntotal, p.nq = nq, p.kf = pl.kf;
	p.e2 = (const float *)ws_e2.p, p.gslot = (unsigned *)ws_gthr.p, p.st = st;
	// (the bound table: the d <= 128 scan, and the big lists' pass A on every store)
	p.pbnd = (pl.wide && !pl.bigk) ? nullptr : (float *)ws_pbnd.p;
	if (pl.bigk) {
		CollectBigRanges r;
		r.ranges = pl.bk_ranges, r.rows = pl.bk_rows;
		if (pl.bk_seed) {
			r.stage = (float *)ws_seed.p;
			launch_collect_big_bounds_seed(p, r);
		} else
			launch_collect_big_bounds(p, r);
	} else {
		CollectPrepare pr;
		pr.stream_cnt = &w.ctl->count, pr.cnt_zeroed = true, pr.slots_ready = !pl.wide;
		pr.seed_stage = pl.wide ? nullptr : (float *)ws_seed.p;
		launch_collect_prepare(p, pr);
	}
}

// One scan of the store into the candidate stream, timed as the search's dominant kernel, and the outlier rows behind it
void FlatIndex::collect_launch_scan(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w) {
	const int64_t nq = rq.nq;
	hipStream_t st = rq.st;
	begin_kernel_timing(st);
	if (pl.few) {
		// Small batches are bound by streaming the bf16 store, not by the matrix pipe: the one-wavefront-per-segment kernel of
		// the IVF scan (csrc/ivf_collect.hip: the database as one list, identity query map, gamma = 0) keeps more bytes in
		// flight per CU than two 256-thread workgroups do
		const int nit = (int)((nq + 127) / 128), seg_rows = 2048;
		const int nseg = (int)((ntotal + seg_rows - 1) / seg_rows);
		const size_t it_bytes = 256, q_bytes = up256((size_t)nq * 4), g_bytes = (size_t)nit * 128 * sizeof(float);
		ws_items1.reserve(it_bytes + 256 + q_bytes + g_bytes);
		char *b = (char *)ws_items1.p;
		int *nitems_dev = (int *)(b + it_bytes);
		int *qidx = (int *)(b + it_bytes + 256);
		float *gam = (float *)(b + it_bytes + 256 + q_bytes);
		MVS_HIP(hipMemsetAsync(gam, 0, g_bytes, st));
		launch_collect_flat_items(b, nitems_dev, qidx, nq, ntotal, st);
		IvfItemSet it;
		it.items = b, it.nitems = nitems_dev, it.max_items = nit, it.qidx = qidx, it.xi = ws_pfq.p, it.igamma = gam, it.ie2 = (float *)ws_e2.p;
		IvfListScan sc;
		sc.rows_bf = vecs_h1(), sc.beta = beta_h1(), sc.gslot = (unsigned *)ws_gthr.p, sc.kk = pl.kf;
		sc.seg_rows = seg_rows, sc.nseg = nseg, sc.collect = 1, sc.rowmask = (const unsigned *)w.pass.rowmask;
		CandStream out = collect_stream(w);
		out.values = nullptr; // (no finish of the small-batch path reads per-entry values)
		launch_ivf_collect_scan(it, sc, out, st);
		w.grid = nit * nseg;
		w.nsplit = nseg;
		w.lds = 20544;
	} else {
		const CollectScanInfo info = launch_collect_scan(w.pass, collect_stream(w), pl.bigk);
		w.grid = info.grid, w.nsplit = info.nsplit, w.lds = info.lds, w.items = info.items;
		cl_scan_items = w.items, cl_scan_ranges = w.nsplit;
	}
	end_kernel_timing(st);
	if (h1_outliers > 0) // the rows kept out of the store join every query's candidates (csrc/flat_collect.hip "outlier rows")
		launch_collect_append_outliers(d_outl.get(), h1_outliers, nq, collect_stream(w), w.pass.rowmask, st);
}

void FlatIndex::ensure_report() {
	report_mem.reserve(sizeof(CollectReport));
}

void FlatIndex::ensure_ctl_copy() {
	cl_hdr_mem.reserve(sizeof(CollectCtl));
}

// the candidates per query of this search size the next one's sort
void FlatIndex::record_candidates(int64_t nq, int64_t ncand) {
	cl_last_candidates = ncand;
	cl_est_per_query = (double)ncand / (double)std::max<int64_t>(nq, 1) + 1e-6;
}

// The scan, and what happens when the stream overflows.  false: the coarse filter gives the batch up (the caller's fall-back takes it).
bool FlatIndex::collect_scan(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res) {
	const int64_t nq = rq.nq;
	hipStream_t st = rq.st;
	for (int attempt = 0;; ++attempt) {
		collect_launch_scan(rq, pl, w);
		ensure_report();
		res.report_cnt = w.defer && cl_est_per_query > 0; // (deferred: the caller's report kernel carries the count, no copy of its own)
		if (!res.report_cnt)
			MVS_HIP(hipMemcpyAsync(&h_report()->candidates, &w.ctl->count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		if (res.report_cnt) { // the caller looks at the count after its own synchronisation
			// (size of the sort: collect_sort_estimate of what the previous search of this index produced per query, in units of 64 K entries)
			res.deferred_cap = pl.fb ? w.cap_entries : std::min<int64_t>(w.cap_entries, collect_sort_estimate(cl_est_per_query, nq)); // (no sort to size)
			return true;
		}
		w.defer = false; // (the first search of an index has no estimate yet: the synchronous way, which leaves one)
		MVS_HIP(hipStreamSynchronize(st));
		w.ncand = (int64_t)h_report()->candidates;
		cl_last_candidates = w.ncand;
		if (w.ncand <= w.cap_entries)
			break;
		// The stream overflowed.  Usually a FEW queries are responsible (a query that sits on a vector stored thousands of times:
		// every copy is a candidate, rightly).  Round 2 handed the whole batch to the bf16x3 / f32 kernels (a 4-11x cliff, VERDICT r2
		// weak #5); now the queries that hold more than their share of the stream are taken out of the coarse filter (2E = NaN:
		// nothing of theirs passes; they join the fail list and are re-run on the exact kernel) and the scan runs once more for
		// the others, with the class slots already warm.  If nobody stands out, or the second scan overflows too: as before.
		++cl_overflows;
		if (attempt > 0 || pl.few)
			return false;
		if (!collect_relieve_overflow(rq, pl, w))
			return false;
		MVS_HIP(hipMemsetAsync(w.ctl, 0, offsetof(CollectCtl, units), st)); // count and kept
	}
	cl_queries_total += nq;
	cl_candidates_total += w.ncand;
	record_candidates(nq, w.ncand);
	return true; // (res.deferred_cap = 0 tells the caller that this pass was synchronous)
}

// Between an overflowed scan and its repetition: a larger stream, or the heavy queries out of it.  false: neither helps.
bool FlatIndex::collect_relieve_overflow(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w) {
	const int64_t nq = rq.nq, ncand = w.ncand;
	const int64_t grow_max = cl_stream_cap_per_query > 0 ? 4 * (int64_t)cl_stream_cap_per_query : std::max<int64_t>(16384, pl.bigk ? 64 * (int64_t)pl.kf : 0);
	if (pl.bigk && (ncand + ncand / 8 > nq * grow_max || ncand + ncand / 8 >= ((int64_t)1 << 31)))
		return false; // (frozen bounds: no query can be taken out of this scan -- the exact kernels take the batch)
	if (ncand + ncand / 8 <= nq * grow_max) {
		// (a) the data simply admits more rows per query than the stream was sized for: a larger stream, one more scan (the
		// class slots are warm: it admits no more than the first), and the next search of this index starts with that size
		w.cap_entries = ncand + ncand / 8;
		if (cl_stream_cap_per_query <= 0)
			cl_cap_hint = std::max<int64_t>(cl_cap_hint, (w.cap_entries + nq - 1) / nq);
		collect_workspaces(pl, nq, w); // (a DevBuf keeps nothing when it grows: the counter -- in ws_seg -- is reset by the caller anyway)
		return true;
	}
	// (b) a few queries hold far more than their share: out of the coarse filter with them, one more scan for the others
	ws_qcount.reserve((size_t)(nq + 16) * sizeof(int));
	MVS_HIP(hipMemsetAsync(ws_qcount.p, 0, (size_t)(nq + 16) * sizeof(int), rq.st));
	const int64_t share = std::max<int64_t>(1, w.cap_entries / nq);
	CollectDropHeavy h;
	h.stream = w.stream, h.n = w.cap_entries, h.nq = nq, h.share = (int)std::min<int64_t>(4 * share, 1 << 30);
	h.qcount = (int *)ws_qcount.p, h.e2 = (float *)ws_e2.p, h.fail = {rq.fail_cnt, rq.fail_q};
	const int nheavy = launch_collect_drop_heavy(h, rq.st); // (syncs the stream)
	if (nheavy <= 0 || nheavy > nq / 2)
		return false;
	cl_heavy_total += nheavy;
	return true;
}

// A query had bmax survivors for a bucket of cl_fpitch entries: a quarter more than that, in units of 64, from now on (the index
// remembers it).  false: beyond 16 384 per query the sorted pipeline takes this index for good.
bool FlatIndex::grow_bucket_pitch(int64_t bmax, int64_t nq) {
	const int64_t want = (bmax + bmax / 4 + 63) / 64 * 64;
	if (want > 16384 || nq * want >= ((int64_t)1 << 31)) {
		cl_fbucket_off = true;
		return false;
	}
	cl_fpitch = (int)want;
	return true;
}

// Bucketed finish: final bound -> survivors into the queries' row buckets -> exact values (FAISS's BLAS-branch formula, or the per-pair
// sum with a selector / fewer than 20 queries) -> selection, FAISS's order, labels: straight into the caller's arrays.
// false: a bucket beyond the largest pitch (the sorted pipeline finishes this pass, and every later one).
bool FlatIndex::collect_finish_bucketed(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res) {
	const int64_t nq = rq.nq;
	hipStream_t st = rq.st;
	unsigned *bcount = (unsigned *)w.seg; // (zero: the preparation kernel / the memset; the select kernel leaves it zero)
	launch_collect_final_thr(w.pass, w.fb_thr);
	ensure_ctl_copy();
	for (;;) {
		IvfFinalBound fb; // (no class slots: the thresholds are there already)
		fb.nq = nq, fb.bf = w.fb_thr;
		IvfRowBuckets rb;
		rb.brow = w.fb_rows, rb.bcount = bcount, rb.bpitch = cl_fpitch, rb.kept_blk = w.fb_kept, rb.units = w.fb_units, rb.unit_cnt = &w.ctl->units;
		launch_ivf_bucket_scatter(collect_stream(w), fb, rb, st);
		IvfBucketFinish f;
		f.metric = metric, f.nq = nq;
		f.ncand = w.cap_entries;
		f.brow = w.fb_rows, f.units = w.fb_units, f.unit_cnt = &w.ctl->units;
		f.x = rq.d_x, f.d = d, f.rows = vecs(), f.dp = geom.dp, f.rows_interleaved = geom.pair_interleaved ? 1 : 0;
		f.bucket = w.fb_keys, f.bcount = bcount, f.bpitch = cl_fpitch;
		f.kk = rq.kk;
		f.stats = &w.ctl->bucket_stats;
		f.kept_blk = w.fb_kept, f.nkept_blk = (int)ivf_bucket_scatter_blocks(w.cap_entries), f.kept_out = &w.ctl->kept;
		IpFlatEmit ipf;
		IvfFlatArith fa;
		if (metric == METRIC_IP) { // the k-ordered chain either way (fvec_inner_product = the BLAS-branch oracle arithmetic)
			memset(&ipf, 0, sizeof ipf);
			if (rq.flags)
				ipf.flags = *rq.flags;
			ipf.kout = rq.kout, ipf.D = rq.D, ipf.I = (long long *)rq.I;
			ipf.idmap = (const long long *)rq.map, ipf.label_offset = rq.off;
			// (reset = false: the per-query counts stay for the tie pass -- FlatIndex::resolve_ip_ties reads A_k off the buckets; the
			// next search's preparation zeroes them)
			res.tie.bucket = w.fb_keys, res.tie.bcount = bcount, res.tie.bpitch = cl_fpitch;
			f.ipf = &ipf, f.reset = false;
		} else {
			memset(&fa, 0, sizeof fa);
			if (!(pl.has_sel || nq < 20))
				fa.qn = (const float *)ws_qn.p, fa.yn = norms();
			f.fa = &fa, f.reset = true;
			f.pd = rq.D, f.pi = rq.I, f.idmap = rq.map, f.label_offset = rq.off;
		}
		launch_ivf_bucket_finish(f, st);
		if (w.defer) // (the caller looks at the header behind its own synchronisation: its report kernel copies it)
			return true;
		MVS_HIP(hipMemcpyAsync(h_cl_hdr(), w.ctl, sizeof(CollectCtl), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		const int64_t bmax = (int64_t)h_cl_hdr()->bucket_max;
		if (bmax <= cl_fpitch)
			return true;
		// some query has more survivors than its bucket holds: a larger pitch and the finish once more -- the scan's stream and values
		// are still there
		if (!grow_bucket_pitch(bmax, nq)) {
			res.tie = TieSource();
			return false;
		}
		collect_workspaces(pl, nq, w);
		// kept / unit counts, statistics, the bucket counters
		MVS_HIP(hipMemsetAsync(&w.ctl->kept, 0, sizeof(CollectCtl) - offsetof(CollectCtl, kept) + (size_t)nq * sizeof(int), st));
		if (rq.flags) // (inner product: the tie flags of the abandoned finish were taken from truncated buckets)
			MVS_HIP(hipMemsetAsync(rq.flags->count, 0, sizeof(int), st));
	}
}

// The sorted pipeline: the stream grouped by query, re-scored exactly, the kk best per query selected into ws_ex -- with the final-bound
// filter in front of the sort where the plan says so (filter-then-sort, the wide big kernel)
void FlatIndex::collect_finish_sorted(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res) {
	const int64_t nq = rq.nq, ncand = w.ncand;
	const int kk = rq.kk;
	hipStream_t st = rq.st;
	// (the filtered stream is sorted in device-count mode whatever the count mode of the scan was)
	size_t temp = (w.defer || pl.wrf) ? collect_sort_temp_bytes_est(w.defer ? res.deferred_cap : std::max<int64_t>(ncand, 1), nq)
	                                  : (ncand > 0 ? collect_sort_temp_bytes(ncand, nq) : 0);
	if (kk > 128 && ncand > 0) // (the selection of a big list is a segmented sort of the exact keys)
		temp = std::max(temp, collect_select_big_temp_bytes(ncand, nq));
	ws_sorttmp.reserve(std::max<size_t>(temp, 16));
	const size_t ex_bytes = up256((size_t)nq * kk * sizeof(float));
	ws_ex.reserve(ex_bytes + (size_t)nq * kk * sizeof(int32_t));
	res.pd1 = (float *)ws_ex.p;
	res.pi1 = (int32_t *)((char *)ws_ex.p + ex_bytes);
	CollectRescore rs;
	rs.metric = metric, rs.temp = ws_sorttmp.p, rs.temp_bytes = temp, rs.seg = w.seg, rs.seg_zeroed = true, rs.nq = nq, rs.kk = kk;
	rs.x = rq.d_x, rs.g = geom, rs.vecs = vecs(), rs.norms = norms(), rs.qn = (const float *)ws_qn.p;
	// (with a selector or fewer than 20 queries FAISS takes its per-pair branch: L2 = sum (x_k - y_k)^2; inner product is the
	// same chain either way)
	rs.per_pair = pl.has_sel || nq < 20;
	rs.pd1 = res.pd1, rs.pi1 = res.pi1;
	if (pl.wrf) {
		// stream -> (filter) -> `sorted` -> (sort by query) -> stream: the survivors' count lives in CollectCtl::kept
		launch_collect_final_thr(w.pass, w.fb_thr);
		launch_stream_refilter(collect_stream(w), w.fb_thr, w.sorted, &w.ctl->kept, st);
		rs.stream = w.sorted, rs.sorted = w.stream, rs.cnt = &w.ctl->kept;
		rs.ncand = w.defer ? res.deferred_cap : std::max<int64_t>(ncand, 1);
		launch_collect_rescore(rs, st);
		res.tie.sorted = w.stream;
		res.filtered = true;
		ensure_ctl_copy();
		if (!res.report_cnt) // (synchronous count mode: the caller's report kernel does not carry the header)
			MVS_HIP(hipMemcpyAsync(h_cl_hdr(), w.ctl, sizeof(CollectCtl), hipMemcpyDeviceToHost, st));
	} else {
		rs.stream = w.stream, rs.sorted = w.sorted, rs.cnt = w.defer ? &w.ctl->count : nullptr;
		rs.ncand = w.defer ? res.deferred_cap : ncand;
		launch_collect_rescore(rs, st);
		res.tie.sorted = w.sorted;
	}
}

// Coarse filter front half (csrc/flat_collect.hip): bound estimation pre-pass, the scan, candidates grouped by query and re-scored
// exactly.  Leaves the kk best exact candidates per query in pd1 / pi1 ([nq][kk]) -- or the final lists in the request's D / I -- and
// the queries whose bound is not finite in fail_q.  !ok: the candidate stream overflowed (the caller uses the bf16x3 path instead).
CollectResult FlatIndex::collect_candidates(const CollectRequest &rq) {
	CollectResult res;
	hipStream_t st = rq.st;
	CollectWork w;
	ensure_h1_rows(st);
	CollectPlan pl = collect_plan(rq);
	// IDSelector: one bit per row, built per search (the selector sees idmap[row] behind an IndexIDMap, the row number else)
	if (pl.has_sel) {
		SelectorDev sel = selector.upload(rq.params, sel_domain(rq.d_idmap), st);
		ws_rowmask.reserve(collect_rowmask_bytes(ntotal));
		launch_collect_rowmask(sel, rq.d_idmap, ntotal, (unsigned long long *)ws_rowmask.p, st);
		w.pass.rowmask = (const unsigned long long *)ws_rowmask.p;
	}
	if (!pl.ok)
		return res;
	// the int8 store serves the scan, its pre-passes and the big lists' pass A (not the small-batch path: csrc/ivf_collect.hip reads bf16)
	const bool use_i8 = !pl.wide && !pl.few && ensure_i8_rows(st);
	w.pass.i8_unit = use_i8 ? i8_unit : 0.f;
	w.pass.rows = use_i8 ? (const unsigned short *)vecs_i8() : vecs_h1();
	w.pass.beta = use_i8 ? (const float *)beta_i8() : beta_h1();
	// the class slots of the pass: the int8 store keeps 32 from k = 15 on (csrc/flat_collect.hip collect_slot_stride)
	w.pass.g = geom, w.pass.kf = pl.kf, w.pass.classes = cl_classes;
	if (!pl.bigk && !pl.few)
		pl.stride = collect_pass_stride(w.pass);
	cl_row_classes = pl.bigk ? 0 : pl.stride;
	w.defer = rq.defer_count && !pl.bigk; // (big lists: the candidate count sizes the sort, read back behind the scan)
	collect_prepare(rq, pl, w);
	if (!collect_scan(rq, pl, w, res))
		return res;
	if (pl.fb && collect_finish_bucketed(rq, pl, w, res)) {
		res.emitted = true;
	} else {
		if (pl.fb && rq.flags) // (the sorted pipeline flags the boundary ties itself)
			MVS_HIP(hipMemsetAsync(rq.flags->count, 0, sizeof(int), st));
		collect_finish_sorted(rq, pl, w, res);
	}
	// one pass over the bf16 store (row pitch of the store + the row's f32 term) + the queries + the results
	set_kinfo(pl.wide ? collect_wide_kernel_name(pl.dp1) : "flat_bf16_collect_kernel", 2.0 * (double)rq.nq * (double)ntotal * d,
	          (double)ntotal * (pl.dp1 * 2.0 + 4.0) + (double)rq.nq * d * 4.0 + (double)rq.nq * rq.kk * 12.0, w.grid, pl.few ? 64 : 256, w.lds,
	          w.nsplit);
	res.ok = true;
	return res;
}

// ---- the search around it ----------------------------------------------------------------------------------------------------------------

// BLAS-branch search through the coarse filter or the bf16x3 prefilter (csrc/flat_bf16.hip).  Returns false when the shape is not served
// (the caller then runs the exact f32 kernel).
bool FlatIndex::search_prefilter(const FlatSearchRequest &r) {
	// First pass: nothing between the scan and the re-scoring waits for the host (the candidate count stays on the device).  If the
	// count, read after the search's own synchronisation, shows that the stream overflowed, the search runs again the round-3 way:
	// count read back behind the scan, stream grown or the heavy queries taken out, scan repeated.
	bool overflow = false;
	const bool ok = search_prefilter_pass(r, cl_defer, &overflow);
	if (!overflow)
		return ok;
	return search_prefilter_pass(r, false, &overflow);
}

// Which of the two filters may take a search
struct PrefilterRoute {
	bool has_sel;
	bool cl_only;    // only the coarse filter exists for this geometry
	int64_t kf;      // the k the coarse FILTER works with
	bool bigk_ok;    // ... on its big-list path (kf > 128)
	bool collect_ok; // the coarse filter serves the shape
};

// false: neither filter serves this search (the exact kernels)
bool FlatIndex::prefilter_route(const FlatSearchRequest &rq, PrefilterRoute &r) const {
	const int64_t nq = rq.nq, k_user = rq.k_user, kk = rq.kk;
	// 128 < d <= 1024: only the coarse filter exists (csrc/flat_collect_wide.hip; no bf16x3 behind it)
	const bool wide = collect_store_dims(d) > 128;
	// (16 < d <= 32: the coarse filter only, as for the wide stores)
	r.cl_only = wide || !prefilter_supported(geom);
	// The coarse FILTER works with the user's k even when the search carries one entry more for the inner-product tie detection
	// (kk = k_user + 1): a row tied with the k-th score passes any bound derived from k rows -- the bound is on values -- so the
	// (k + 1)-th entry of the SELECTION is a tied row if there is one.  The bound is then the k-th, not the (k + 1)-th, best class,
	// and k = 32 / k = 16 stay on the 32- / 16-class instances (wide stores: k = 32 stays on the filter at all) -- ADVICE r3, low.
	const int64_t kf = r.kf = kk > k_user ? k_user : kk;
	const int cl_kmax0 = cl_k32 ? collect_max_k(d) : std::min(16, collect_max_k(d)); // 32 row classes at d <= 128 (option cl_k32), else 16
	const bool filter_on = prefilter_mode == 2 || prefilter_mode < 0; // (mode 2 forces the coarse filter, auto prefers it where its kernel exists)
	// (round 6: beyond 128 entries the d <= 128 store's filter takes its bounds from a pass of its own and selects by a segmented sort --
	// CollectPlan::bigk; option cl_bigk = 0: the exact kernels as before)
	r.bigk_ok = cl_bigk && (!wide || collect_wide_max_classes(collect_store_dims(d)) >= 128) && collect_supported(geom) && kf > 128 - (kk - kf) &&
	            kk <= std::min<int64_t>(wide ? 2049 : 4097, flat_direct_max_k()) /* (what the fall-back can serve) */ && ntotal >= 65536 &&
	            ntotal >= 64 * kf && ntotal < ((int64_t)1 << 31) && filter_on && nq * kk < ((int64_t)1 << 31);
	const int cl_kmax = r.bigk_ok ? 4096 : (int)std::min<int64_t>(cl_kmax0, 128 - (kk - kf)); // (collect_select_kernel: kk <= 128 entries)
	r.collect_ok = filter_on && collect_supported(geom) && kf <= cl_kmax;
	// (lists beyond 40: only the coarse filter of the d <= 128 store, up to 128 -- four subsets of 32 row classes, round 4)
	if (prefilter_mode == 0 || rq.exact_only || (!prefilter_supported(geom) && !collect_supported(geom)) || (kk > 40 && kf > cl_kmax))
		return false;
	// an IDSelector: only the coarse filter handles it (SEL instances); otherwise the exact kernels' SEL instances do
	r.has_sel = rq.has_sel();
	if (r.cl_only && (kf > (r.bigk_ok ? 4096 : std::min<int64_t>(collect_max_k(d), 128 - (kk - kf))) || prefilter_mode == 1))
		return false;
	if (r.has_sel && !r.collect_ok)
		return false;
	// auto: the contraction must dominate.  The coarse filter wins from FAISS's first BLAS-branch batch on (N = 10M: 1.3 ms vs
	// 3.5 ms at 64 queries, 1.7 vs 11.0 at 500); the bf16x3 kernel needs whole 256-query blocks to pay
	// (N = 131 072: 0.35 vs 0.46 ms at 64 queries, 1.36 vs 3.88 at 10k; N = 65 536: 1.40 vs 2.25 at 10k but 1.07 vs 0.61 at 2048;
	// below that the f32 kernel's ~0.3 ms wins everywhere)
	const bool big_enough = ntotal >= 262144 || (r.collect_ok && ntotal >= 65536 && (double)nq * (double)ntotal >= 5e8) ||
	                        (r.collect_ok && ntotal >= 131072 && nq <= 128);
	if (prefilter_mode < 0 && (!big_enough || (nq < 512 && !r.collect_ok)))
		return false;
	if (nq < 20 && !r.collect_ok) // (FAISS's per-pair branch: only the coarse filter re-scores in that arithmetic)
		return false;
	return ntotal >= 4096 && ntotal > kk;
}

// The bf16x3 prefilter: approximate top-kp per query, their exact values and the per-query proof (queries it cannot prove join fail_q).
// Leaves [nq][kp] exact candidates in ws_ex (cr.pd1 / cr.pi1) and returns kp.
int FlatIndex::prefilter_bf16x3(const FlatSearchRequest &r, int *fail_cnt, int *fail_q, CollectResult &cr) {
	const int64_t nq = r.nq, kk = r.kk;
	hipStream_t st = r.st;
	// candidates per query (<= 64: one lane each in the proof).  The margin sets how often a query cannot be proven: at the
	// headline (N = 10M, d = 128) 5 spare ranks leave ~3 of 10 000 queries to the exact kernel, 8 spare ranks ~none
	constexpr int64_t margin = 6;
	int kp = (int)(kk + std::max<int64_t>(margin, kk / 2));
	if (kp > 16 && kk + 5 <= 16)
		kp = 16; // one 16-slot window of shared thresholds: a second window costs more than the lost margin (measured: 61 vs 70 ms)
	ensure_bf16_rows(st);
	FlatSearchPlan p = plan_prefilter(geom, nq, ntotal, kp);
	ws_pfq.reserve(prefilter_qfrag_bytes(geom, nq));
	ws_qn.reserve((size_t)nq * sizeof(float));
	launch_pack_queries_bf16(geom, r.d_x, nq, ws_pfq.p, st);
	launch_query_norms(r.d_x, nq, d, (float *)ws_qn.p, st);
	ws_pd.reserve((size_t)p.nsplit * nq * kp * sizeof(float));
	ws_pi.reserve((size_t)p.nsplit * nq * kp * sizeof(int32_t));
	ws_gthr.reserve((size_t)nq * std::max(32, (kp + 15) / 16 * 16) * sizeof(unsigned) + 64);
	begin_kernel_timing(st);
	launch_prefilter(geom, p, metric, ws_pfq.p, (const float *)ws_qn.p, nq, vecs_bf(), norms(), ntotal, kp, (float *)ws_pd.p,
	                 (int32_t *)ws_pi.p, (unsigned *)ws_gthr.p, st);
	end_kernel_timing(st);
	// approximate top-kp per query (plain row numbers)
	const size_t ca_bytes = up256((size_t)nq * kp * sizeof(float));
	ws_cand.reserve(ca_bytes + (size_t)nq * kp * sizeof(int64_t));
	float *ca = (float *)ws_cand.p;
	int64_t *ci = (int64_t *)((char *)ws_cand.p + ca_bytes);
	launch_merge_partials(metric, (const float *)ws_pd.p, (const int32_t *)ws_pi.p, p.nsplit, nq, kp, nullptr, 0, ca, ci, st);
	// exact values of the candidates + the per-query proof
	const size_t ex_bytes = up256((size_t)nq * kp * sizeof(float));
	ws_ex.reserve(ex_bytes + (size_t)nq * kp * sizeof(int32_t));
	cr.pd1 = (float *)ws_ex.p;
	cr.pi1 = (int32_t *)((char *)ws_ex.p + ex_bytes);
	launch_rescore_verify(metric, ca, ci, nq, kp, (int)kk, r.d_x, geom, vecs(), norms(), (const float *)ws_qn.p, d_max_norm_bits.get(), cr.pd1, cr.pi1, fail_cnt,
	                      fail_q, d_max_norm_bits.get() + CL_NORM_REL_ERR, st);
	set_kinfo("flat_bf16x3_kernel", 2.0 * (double)nq * (double)ntotal * d,
	          (double)ntotal * d * 4.0 + (double)nq * d * 4.0 + (double)nq * r.k_user * 12.0, p.grid, 256, (int)p.lds_bytes, p.nsplit);
	return kp;
}

// Deferred count mode, behind the caller's synchronisation: true if the scan produced more entries than the sort / the stream covered
// (the count then sizes the synchronous pass that repeats the search)
bool FlatIndex::deferred_count_overflowed(int64_t nq, int64_t deferred_cap) {
	const int64_t ncand = (int64_t)h_report()->candidates;
	if (ncand <= deferred_cap)
		return false;
	record_candidates(nq, ncand);
	return true;
}

// Behind the synchronisation of a search whose pass succeeded: what the control block's header and the report say about it.
// false: it has to be repeated synchronously -- a bucket or (deferred count mode) the sort was too small for what the scan produced.
bool FlatIndex::collect_settle(const CollectResult &cr, bool deferred, int64_t nq) {
	if (cr.emitted) { // a bucket too small for some query: its list is incomplete -- the sorted pipeline takes over for good
		cl_last_rescored = (int64_t)h_cl_hdr()->kept; // (survivors of the final-bound filter: what the exact stage re-scored)
		if ((int64_t)h_cl_hdr()->bucket_max > cl_fpitch) { // (the synchronous pass grows the pitch itself from there on)
			grow_bucket_pitch((int64_t)h_cl_hdr()->bucket_max, nq);
			return false;
		}
	}
	if (deferred) { // the candidate count of the scan is on the host now
		if (deferred_count_overflowed(nq, cr.deferred_cap))
			return false; // (more entries than the sort covered: the synchronous pass overwrites the results written so far)
		record_candidates(nq, (int64_t)h_report()->candidates);
		cl_queries_total += nq;
		cl_candidates_total += cl_last_candidates;
	}
	if (cr.filtered && !cr.emitted) // (the wide stores' filter: survivors in CollectCtl::kept)
		cl_last_rescored = (int64_t)h_cl_hdr()->kept;
	if ((cr.emitted || cr.filtered) && cl_last_rescored >= 0) // (mvs_index_collect_stats then reports what the exact stage re-scored, as for an IVF index)
		cl_rescored_total += cl_last_rescored, cl_rescored_queries += nq, cl_admitted_in_fb += cl_last_candidates;
	return true;
}

// The queries of `batch` that a filter or the shadow could not prove (fail_q[0 .. nf), on the device), run again through the tie wrapper
// as a quiet request of their own, on the branch FAISS sends their BATCH down (pair_branch); the results overwrite their rows of the
// batch's.  exact_only: a filter's re-run.  Else the shadow's: the coarse filter may take it, and the filters judge a pass by its nq, so
// fewer than 20 queries are padded to 20 with copies of the first (only the first nf results are used).
void FlatIndex::rerun_unproven(const FlatSearchRequest &batch, int nf, int *fail_q, bool exact_only) {
	const int64_t k = batch.k_user;
	hipStream_t st = batch.st;
	const int nr = exact_only ? nf : std::max(nf, 20);
	for (int i = nf; i < nr; ++i)
		MVS_HIP(hipMemcpyAsync(fail_q + i, fail_q, sizeof(int), hipMemcpyDeviceToDevice, st));
	const size_t xf_bytes = up256((size_t)nr * d * sizeof(float));
	const size_t df_bytes = up256((size_t)nr * k * sizeof(float));
	ws_fb.reserve(xf_bytes + df_bytes + (size_t)nr * k * sizeof(int64_t));
	float *xf = (float *)ws_fb.p;
	float *Df = (float *)((char *)ws_fb.p + xf_bytes);
	int64_t *If = (int64_t *)((char *)Df + df_bytes);
	launch_gather_query_rows(batch.d_x, d, fail_q, nr, xf, st);
	FlatSearchRequest in = batch;
	in.nq = nr, in.d_x = xf, in.D = Df, in.I = If;
	in.kk = k, in.flags = nullptr; // (the tie wrapper makes its own k + 1 request: the batch's flags are consumed by now)
	in.exact_only = exact_only, in.no_shadow = in.quiet = true;
	tie_wrapped_search(in);
	launch_scatter_rows(fail_q, nf, k, Df, If, batch.D, batch.I, st);
}

bool FlatIndex::search_prefilter_pass(const FlatSearchRequest &r, bool defer, bool *overflow) {
	const int64_t nq = r.nq, k_user = r.k_user, kk = r.kk;
	const float *const d_x = r.d_x;
	float *const d_D = r.D;
	int64_t *const d_I = r.I;
	const TieFlags *const flp = r.flags;
	hipStream_t st = r.st;
	*overflow = false;
	if (flp) // (a second pass must not see the tie flags the first one recorded from a truncated candidate set)
		MVS_HIP(hipMemsetAsync(flp->count, 0, sizeof(int), st));
	PrefilterRoute rt;
	if (!prefilter_route(r, rt))
		return false;
	// Rows that cluster (round 5): through the shadow IVF index, when one is wanted (see FlatIndex::shadow_search)
	if (metric == METRIC_L2 && !rt.has_sel && !flp && kk == k_user && nq >= 256 && !r.no_shadow && shadow_mode != 0 &&
	    (shadow_state == 1 || shadow_mode == 1) && shadow_search(r))
		return true;
	ws_fail.reserve(64 + (size_t)nq * sizeof(int));
	int *fail_cnt = (int *)ws_fail.p, *fail_q = fail_cnt + 16;
	MVS_HIP(hipMemsetAsync(fail_cnt, 0, sizeof(int), st));
	int kp = 0;
	CollectResult cr;
	// Coarse filter (one bf16 product per pair, candidates by a proven bound); on a stream overflow the bf16x3 path below takes the batch.
	// Data on which the filter gave up (every query sits on thousands of copies of its nearest row: two scans that only count,
	// then the exact kernels anyway) is not asked again at once: the next 4, 8, ... 64 large searches of this index go straight to
	// the fall-back (all-duplicates, N = 2 M: 1.3 s per batch with the two futile scans, 0.07 s without)
	if (rt.collect_ok && cl_skip > 0 && nq >= 20 && !rt.has_sel && !rt.cl_only && kk <= 40) {
		--cl_skip;
	} else if (rt.collect_ok) {
		kp = (int)kk;
		CollectRequest rq {};
		rq.nq = nq, rq.d_x = d_x, rq.kk = kp, rq.kf = (int)(rt.bigk_ok ? std::max<int64_t>(rt.kf, 129) : rt.kf);
		rq.params = r.params, rq.d_idmap = r.d_idmap, rq.fail_cnt = fail_cnt, rq.fail_q = fail_q, rq.defer_count = defer, rq.st = st;
		// (collect_candidates may write the final lists itself: L2 as they are, inner product with the tie flags of this search)
		const bool direct = (metric == METRIC_L2 && !flp && kk == k_user) || (metric == METRIC_IP && kk <= k_user + 1 && (flp || kk == k_user));
		rq.D = direct ? d_D : nullptr, rq.I = direct ? d_I : nullptr, rq.map = r.out_map, rq.off = r.out_off;
		rq.flags = flp, rq.kout = (int)k_user;
		cr = collect_candidates(rq);
		if (!cr.ok) {
			MVS_HIP(hipMemsetAsync(fail_cnt, 0, sizeof(int), st));
			cl_skip_len = std::min(64, std::max(4, 2 * cl_skip_len));
			cl_skip = cl_skip_len;
		} else if (!defer) {
			cl_skip_len = 0;
		}
	}
	const bool collected = cr.ok;
	if (!collected && (rt.has_sel || nq < 20 || rt.cl_only || kk > 40))
		return false; // (stream overflow under a selector / in the per-pair branch / beyond the bf16x3 lists: the exact kernels take the batch)
	if (!collected)
		kp = prefilter_bf16x3(r, fail_cnt, fail_q, cr);
	// the exact candidates through the normal merge: FAISS order, labels, inner-product tie flags
	const bool emitted = cr.emitted; // (the bucketed finish printed the lists already)
	if (emitted)
		;
	else if (collected && metric == METRIC_L2 && !flp) // (the coarse filter's selection is in FAISS's L2 order already: labels only)
		launch_emit_sorted(cr.pd1, cr.pi1, nq, kp, k_user, r.out_map, r.out_off, d_D, d_I, st);
	else
		launch_merge_partials(metric, cr.pd1, cr.pi1, 1, nq, kp, r.out_map, r.out_off, d_D, d_I, st, k_user, flp, collected /* the coarse filter's selection is sorted */);
	ensure_report();
	// (one kernel writes fail count, rounding residual and -- deferred count mode -- the scan's entry count / the control block's header to pinned memory)
	const bool with_hdr = emitted || cr.filtered; // (the host reads CollectCtl::bucket_max / kept of this pass)
	CollectReportSrc rep;
	rep.hdr = collected ? ws_seg.p : nullptr, rep.fail_cnt = fail_cnt, rep.maxnorm = d_max_norm_bits.get() + CL_NORM_REL_ERR;
	rep.h_flags = (int *)h_report(), rep.h_hdr = (with_hdr && cr.report_cnt) ? h_cl_hdr() : nullptr, rep.with_cnt = cr.report_cnt;
	launch_collect_report(rep, st);
	const bool deferred = collected && defer && cr.deferred_cap > 0; // the candidate count of the scan is on the host after the next synchronisation
	if (flp) {
		if (deferred) {
			// (the sort covered deferred_cap entries -- if the scan produced more, the tie pass below would work on a
			// truncated candidate set, for k >= 100 with a full score pass per flagged query, only for the whole search to be repeated)
			MVS_HIP(hipStreamSynchronize(st));
			if (deferred_count_overflowed(nq, cr.deferred_cap)) {
				*overflow = true;
				return false;
			}
		}
		SelectorDev tsel;
		memset(&tsel, 0, sizeof tsel);
		if (rt.has_sel)
			tsel = selector.upload(r.params, sel_domain(r.d_idmap), st);
		// (after the coarse filter the rows at or above the boundary score all are candidates: no second pass over the database.  The key
		// buckets serve lists below 100 entries only -- from k = 100 on the reservoir replay reads scores, not A_k -- which CollectPlan::fb's
		// kk <= 64 guarantees: a bucketed finish of longer lists would have to leave TieSource::bucket null)
		resolve_ip_ties(nq, d_x, k_user, *flp, tsel, r.d_idmap, d_D, d_I, st, kp, collected && tie_from_candidates ? &cr.tie : nullptr); // (syncs the stream)
	} else {
		MVS_HIP(hipStreamSynchronize(st));
	}
	if (!collect_settle(cr, deferred, nq)) { // (synchronised above)
		*overflow = true;
		return false;
	}
	const int nf = h_report()->fail_count;
	pf_last_fallback = nf;
	pf_queries_total += nq;
	pf_fallback_total += nf;
	// the global-centring filter admits thousands of rows per query: this data clusters (or is badly conditioned) -- the next large
	// search goes through a shadow IVF index of the rows (built then; FlatIndex::shadow_search)
	if (collected && !r.no_shadow && shadow_state == 0 && shadow_mode < 0 && metric == METRIC_L2 && !rt.has_sel && nq >= 256 && ntotal >= 262144 && d % 32 == 0 &&
	    d <= 128 && kk <= 32 && cl_last_candidates > 600 * nq)
		shadow_state = 1;
	pf_max_rel_err = h_report()->residual;
	if (nf > 0)
		rerun_unproven(r, nf, fail_q, true);
	return true;
}

} // namespace mvs
