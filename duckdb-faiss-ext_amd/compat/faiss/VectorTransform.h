// compat/faiss/VectorTransform.h -- faiss::VectorTransform and the three kinds the device's pre-transform chain holds (include/mi355_faiss.h
// "pre-transform indexes").  These are VIEWS of slot `slot` of the device index's chain: the matrices live there (mvs_index_pretransform_get_linear
// / _get_pca read them), apply() transforms through the whole device chain only on the owning IndexPreTransform.
#pragma once
#include "Index.h"
#include <vector>
namespace faiss {
struct VectorTransform {
	int d_in = 0, d_out = 0;
	bool is_trained = false;
	mvs_index *handle = nullptr; // the device index whose chain this transform is part of (borrowed)
	int slot = 0;
	virtual ~VectorTransform() {
	}
	void refresh(); // d_in, d_out, is_trained (and have_bias) from the device
};
struct LinearTransform : VectorTransform {
	bool have_bias = false;
	std::vector<float> get_A() const; // [d_out][d_in]
	std::vector<float> get_b() const; // [d_out], zeros without a bias
};
struct PCAMatrix : LinearTransform {
	float eigen_power = 0, epsilon = 0;
	std::vector<float> get_mean() const, get_eigenvalues() const;
};
struct NormalizationTransform : VectorTransform {
	float norm = 2;
};
} // namespace faiss
