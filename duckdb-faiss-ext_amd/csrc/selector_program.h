// csrc/selector_program.h -- the host side of MVS_SEL_PROGRAM (include/mi355_faiss.h "selector programs").  Plain C++, no
// HIP: a stand-alone program compiles it (tests/test_selector_program_cpu.py builds one with the sanitizers), as csrc/remove_plan.h.
//
//   sel_program_validate   the first thing wrong with a caller's nodes, as "node <i>: <reason>", or nothing
//   SelProgram             the packed form: the nodes with every leaf's data in ONE blob (what csrc/selector_lower.hip uploads); id lists
//                          are sorted here, once, so that host and device test them by bisection
//   sel_program_member     the Boolean value of the program for one id: a 64-bit stack of bits, the same walk the device kernel does
#pragma once
#include "../../include/mi355_faiss.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mvs {

constexpr int SEL_PROGRAM_MAX_NODES = 64; // nodes, and so the deepest stack: one 64-bit word per lane holds it

// one node as the device reads it: `off` is the byte offset of the leaf's data in the blob (a multiple of 8)
struct SelPackedNode {
	int32_t op, pad;
	int64_t off, n; // BITMAP: bytes; BATCH / ARRAY: ids (ascending)
	int64_t imin, imax;
};

struct SelProgram {
	std::vector<SelPackedNode> nodes;
	std::vector<uint8_t> blob;
};

inline bool sel_op_is_leaf(int op) {
	return op == MVS_SELOP_ALL || op == MVS_SELOP_BITMAP || op == MVS_SELOP_BATCH || op == MVS_SELOP_ARRAY || op == MVS_SELOP_RANGE;
}

// "" if the program is well formed, else "node <i>: <reason>"
inline std::string sel_program_validate(const mvs_sel_node *nodes, int64_t n) {
	char msg[160];
	auto fail = [&](long long i, const char *fmt, long long a = 0) {
		char why[120];
		snprintf(why, sizeof why, fmt, a);
		snprintf(msg, sizeof msg, "node %lld: %s", i, why);
		return std::string(msg);
	};
	if (n <= 0 || !nodes)
		return fail(0, "the program is empty (%lld nodes)", (long long)std::max<int64_t>(n, 0));
	if (n > SEL_PROGRAM_MAX_NODES)
		return fail(SEL_PROGRAM_MAX_NODES, "more than 64 nodes (%lld)", (long long)n);
	int depth = 0;
	for (int64_t i = 0; i < n; ++i) {
		const mvs_sel_node &nd = nodes[i];
		if (sel_op_is_leaf(nd.op)) {
			if (nd.op == MVS_SELOP_BITMAP || nd.op == MVS_SELOP_BATCH || nd.op == MVS_SELOP_ARRAY) {
				if (nd.n < 0)
					return fail(i, "n < 0 (%lld)", (long long)nd.n);
				if (nd.n > 0 && !nd.data)
					return fail(i, "NULL data with n > 0 (%lld)", (long long)nd.n);
			}
			++depth; // (at most 64 nodes: it cannot pass 64)
		} else if (nd.op == MVS_SELOP_NOT) {
			if (depth < 1)
				return fail(i, "stack underflow (NOT needs one value)");
		} else if (nd.op == MVS_SELOP_AND || nd.op == MVS_SELOP_OR || nd.op == MVS_SELOP_XOR) {
			if (depth < 2)
				return fail(i, "stack underflow (a binary operation needs two values, %lld there)", depth);
			--depth;
		} else {
			return fail(i, "unknown op %lld", (long long)nd.op);
		}
	}
	if (depth != 1)
		return fail(n - 1, "%lld values left on the stack (a program leaves exactly one)", depth);
	return std::string();
}

// nodes must be valid (sel_program_validate)
inline void sel_program_pack(const mvs_sel_node *nodes, int64_t n, SelProgram &out) {
	out.nodes.assign((size_t)n, SelPackedNode {});
	out.blob.clear();
	for (int64_t i = 0; i < n; ++i) {
		const mvs_sel_node &nd = nodes[i];
		SelPackedNode &p = out.nodes[(size_t)i];
		p.op = nd.op;
		p.imin = nd.imin, p.imax = nd.imax;
		p.off = (int64_t)out.blob.size();
		if (nd.op == MVS_SELOP_BITMAP && nd.n > 0) {
			p.n = nd.n;
			out.blob.resize(out.blob.size() + (size_t)((nd.n + 7) & ~(int64_t)7), 0);
			memcpy(out.blob.data() + p.off, nd.data, (size_t)nd.n);
		} else if ((nd.op == MVS_SELOP_BATCH || nd.op == MVS_SELOP_ARRAY) && nd.n > 0) {
			p.n = nd.n;
			std::vector<int64_t> ids((const int64_t *)nd.data, (const int64_t *)nd.data + nd.n);
			std::sort(ids.begin(), ids.end());
			out.blob.resize(out.blob.size() + ids.size() * sizeof(int64_t));
			memcpy(out.blob.data() + p.off, ids.data(), ids.size() * sizeof(int64_t));
		}
	}
}

// one leaf: shared between the host evaluator and (textually the same rules) selector_eval_kernel
inline bool sel_leaf_member(const SelPackedNode &p, const uint8_t *blob, int64_t id) {
	switch (p.op) {
	case MVS_SELOP_ALL:
		return true;
	case MVS_SELOP_RANGE:
		return id >= p.imin && id < p.imax;
	case MVS_SELOP_BITMAP: { // the rule of MVS_SEL_BITMAP: the id read as uint64; beyond the bitmap is no member
		const uint64_t u = (uint64_t)id;
		if ((u >> 3) >= (uint64_t)p.n)
			return false;
		return (blob[p.off + (int64_t)(u >> 3)] >> (u & 7)) & 1;
	}
	default: { // BATCH / ARRAY: bisection of the ascending list (memcpy: the blob is bytes)
		int64_t lo = 0, hi = p.n;
		while (lo < hi) {
			const int64_t mid = lo + ((hi - lo) >> 1);
			int64_t v;
			memcpy(&v, blob + p.off + mid * (int64_t)sizeof(int64_t), sizeof v);
			if (v < id)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo >= p.n)
			return false;
		int64_t v;
		memcpy(&v, blob + p.off + lo * (int64_t)sizeof(int64_t), sizeof v);
		return v == id;
	}
	}
}

inline bool sel_program_member(const SelProgram &prog, int64_t id) {
	uint64_t stk = 0; // bit 0 is the top
	for (const SelPackedNode &p : prog.nodes) {
		if (p.op == MVS_SELOP_NOT) {
			stk ^= 1;
		} else if (p.op == MVS_SELOP_AND || p.op == MVS_SELOP_OR || p.op == MVS_SELOP_XOR) {
			const uint64_t b = stk & 1;
			stk >>= 1;
			const uint64_t a = stk & 1;
			const uint64_t r = p.op == MVS_SELOP_AND ? (a & b) : p.op == MVS_SELOP_OR ? (a | b) : (a ^ b);
			stk = (stk & ~(uint64_t)1) | r;
		} else {
			stk = (stk << 1) | (sel_leaf_member(p, prog.blob.data(), id) ? 1u : 0u);
		}
	}
	return stk & 1;
}

} // namespace mvs
