// csrc/clustering.hip -- faiss::Clustering::train on the device: kmeans_train (csrc/index.h; DESIGN.md 3.16 names the callers).  No kernel.
// Restated FAISS behaviour [UPSTREAM: faiss/Clustering.cpp, utils/random.cpp; oracle/orc_core.c restates it line by line]: seed 1234, <= 256
// points per centroid (subsample via rand_perm), centroids initialised from rand_perm(seed + 1), empty-cluster splitting, unit-norm centroids
// when spherical.  The ASSIGNMENT step -- 11 TFLOP at IVF4096 -- is the assigner's k = 1 search (the fused MFMA Flat kernel); the centroid
// update keeps FAISS's sequential summation order on the device too (stable sort by assignment + one thread per (centroid, dim),
// csrc/kmeans_update.hip); the host only replays the RNG-driven empty-cluster splits on k x d values.
#include "index.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <random>
#include <thread>

namespace mvs {

namespace {

// faiss::rand_perm (utils/random.cpp): Fisher-Yates with mt19937, i2 = i + rng() % (n - i)
std::vector<int> rand_perm(size_t n, int64_t seed) {
	std::vector<int> perm(n);
	for (size_t i = 0; i < n; i++)
		perm[i] = (int)i;
	std::mt19937 mt((unsigned)seed);
	for (size_t i = 0; i + 1 < n; i++) {
		int i2 = (int)i + (int)(mt() % (uint32_t)(n - i));
		std::swap(perm[i], perm[i2]);
	}
	return perm;
}

float chain_norm(const float *x, int d) {
	float acc = 0.f;
	for (int k = 0; k < d; k++)
		acc = fmaf(x[k], x[k], acc);
	return acc;
}
void renorm_l2(int d, int64_t n, float *x) {
	for (int64_t i = 0; i < n; i++) {
		float *xi = x + i * d;
		float nr = chain_norm(xi, d);
		if (nr > 0) {
			const float inv = 1.0f / sqrtf(nr);
			for (int j = 0; j < d; j++)
				xi[j] *= inv;
		}
	}
}

} // namespace

void kmeans_train(const KMeansSpec &s, int64_t nx, const float *x_in, FlatIndex &assigner) {
	// Clustering defaults (faiss/Clustering.h); niter is the caller's (Level1Quantizer's constructor sets cp.niter = 10 for every IndexIVF)
	FlatIndex *const qz = &assigner;
	qz->use_device();
	const hipStream_t stream = qz->stream;
	const bool spherical = s.spherical;
	const int d = qz->d, niter = s.niter, max_pts = 256, min_pts = 39;
	const int64_t seed = 1234, k = s.k;
	if (nx < k)
		throw_faiss("virtual void faiss::Clustering::train_encoded(...)", "faiss/Clustering.cpp",
		            "Error: 'nx >= k' failed: Number of training points (%ld) should be at least as large as number "
		            "of clusters (%ld)",
		            (long)nx, (long)k);
	{
		// FAISS checks EVERY training value on the host (faiss/Clustering.cpp); 1.28 G values at C3's ingest: split over threads
		const int64_t tot = nx * d;
		const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, std::min<int64_t>(std::thread::hardware_concurrency(), tot >> 22)));
		std::atomic<bool> bad(false);
		auto scan = [&](int64_t b, int64_t e) {
			bool ok = true;
			for (int64_t i = b; i < e && ok; i += 4096) {
				const int64_t m = std::min<int64_t>(e, i + 4096);
				float acc = 0.f; // (x * 0 is 0 for every finite x, NaN otherwise: a branch-free pass the compiler vectorises)
				for (int64_t j = i; j < m; ++j)
					acc += x_in[j] * 0.0f;
				ok = acc == 0.f;
			}
			if (!ok)
				bad.store(true);
		};
		std::vector<std::thread> th;
		for (int t = 1; t < nt; ++t)
			th.emplace_back(scan, tot * t / nt, tot * (t + 1) / nt);
		scan(0, tot / nt);
		for (auto &t : th)
			t.join();
		if (bad.load())
			throw_faiss("virtual void faiss::Clustering::train_encoded(...)", "faiss/Clustering.cpp",
			            "input contains NaN's or Inf's");
	}
	std::vector<float> sub;
	const float *x = x_in;
	if (nx > k * max_pts) { // subsample_training_set
		std::vector<int> perm = rand_perm((size_t)nx, seed);
		const int64_t n2 = k * max_pts;
		sub.resize((size_t)n2 * d);
		for (int64_t i = 0; i < n2; i++)
			memcpy(&sub[(size_t)i * d], x_in + (int64_t)perm[i] * d, (size_t)d * sizeof(float));
		x = sub.data();
		nx = n2;
	} else if (nx < k * min_pts) {
		fprintf(stderr, "WARNING clustering %ld points to %ld centroids: please provide at least %ld training points\n",
		        (long)nx, (long)k, (long)(k * min_pts));
	}
	std::vector<float> cent((size_t)k * d);
	if (nx == k) {
		memcpy(cent.data(), x, cent.size() * sizeof(float));
		qz->reset();
		qz->add(k, cent.data());
		return;
	}
	{
		std::vector<int> perm = rand_perm((size_t)nx, seed + 1);
		for (int64_t i = 0; i < k; i++)
			memcpy(&cent[(size_t)i * d], x + (int64_t)perm[i] * d, (size_t)d * sizeof(float));
	}
	if (spherical)
		renorm_l2(d, k, cent.data());
	qz->reset();
	qz->add(k, cent.data());

	// the training sample lives on device for the assignment passes
	DevBuf dx, dD, dI;
	dx.reserve((size_t)nx * d * sizeof(float));
	dD.reserve((size_t)nx * sizeof(float));
	dI.reserve((size_t)nx * sizeof(int64_t));
	MVS_HIP(hipMemcpyAsync(dx.p, x, (size_t)nx * d * sizeof(float), hipMemcpyHostToDevice, stream));
	std::vector<float> hassign((size_t)k);
	DevBuf dcent, dhass, dws;
	dcent.reserve((size_t)k * d * sizeof(float));
	dhass.reserve((size_t)k * sizeof(float));
	const size_t wsb = kmeans_update_ws_bytes(nx, k);
	dws.reserve(wsb);
	for (int it = 0; it < niter; it++) {
		// (round 6: the assignment is a Flat search with k = 1 over a few thousand rows -- csrc/coarse_bf16.hip serves it, same labels)
		if (!qz->coarse_topk(nx, (const float *)dx.p, 1, (float *)dD.p, (int64_t *)dI.p, stream, false))
			qz->search_device(nx, (const float *)dx.p, 1, (float *)dD.p, (int64_t *)dI.p, nullptr, stream);
		qz->use_device();
		// compute_centroids on device in FAISS's summation order (csrc/kmeans_update.hip); only the k x d
		// centroids and the k counts come back for the (rare, RNG-driven) empty-cluster splits
		launch_kmeans_update((const float *)dx.p, nx, d, (const int64_t *)dI.p, k, (float *)dcent.p, (float *)dhass.p,
		                     dws.p, wsb, stream);
		MVS_HIP(hipMemcpyAsync(cent.data(), dcent.p, cent.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipMemcpyAsync(hassign.data(), dhass.p, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		{
			double counted = 0;
			for (float h : hassign)
				counted += h;
			if ((int64_t)counted != nx) // compute_centroids: FAISS_ASSERT(ci >= 0 && ci < k)
				throw_faiss("void faiss::compute_centroids(...)", "faiss/Clustering.cpp",
				            "Error: 'ci >= 0 && ci < k' failed: %lld of %lld training points have no finite nearest "
				            "centroid (distance overflow)",
				            (long long)(nx - (int64_t)counted), (long long)nx);
		}
		// split_clusters
		{
			const float EPS = (float)(1 / 1024.);
			std::mt19937 mt(1234);
			for (int64_t ci = 0; ci < k; ci++) {
				if (hassign[(size_t)ci] != 0)
					continue;
				int64_t cj;
				for (cj = 0;; cj = (cj + 1) % k) {
					const float p = (hassign[(size_t)cj] - 1.0f) / (float)(nx - k);
					const float r = (float)mt() / (float)mt.max();
					if (r < p)
						break;
				}
				memcpy(&cent[(size_t)ci * d], &cent[(size_t)cj * d], (size_t)d * sizeof(float));
				for (int j = 0; j < d; j++) {
					if (j % 2 == 0) {
						cent[(size_t)ci * d + j] *= 1 + EPS;
						cent[(size_t)cj * d + j] *= 1 - EPS;
					} else {
						cent[(size_t)ci * d + j] *= 1 - EPS;
						cent[(size_t)cj * d + j] *= 1 + EPS;
					}
				}
				hassign[(size_t)ci] = hassign[(size_t)cj] / 2;
				hassign[(size_t)cj] -= hassign[(size_t)ci];
			}
		}
		if (spherical)
			renorm_l2(d, k, cent.data());
		qz->reset();
		qz->add(k, cent.data());
	}
}

} // namespace mvs
