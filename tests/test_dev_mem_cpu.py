"""The owners of device memory (csrc/dev_mem.h: DevMem, DevBuf, DevBlock, DevKeep, DevRowStore) and of pinned memory (PinnedMem) on the host heap: a stand-alone C++ program, built
here with AddressSanitizer and UBSan against the header's host mode (MVS_DEV_MEM_HOST) and run as a process of its own (nothing is loaded
into Python).  With rows of 8 bytes, side values of 4, a padding of 3 rows and 5 to 40 rows it checks that a growth keeps the converted
prefix bit for bit and leaves every other byte zero, the padding included; that a failure of the first allocation, and then of the second,
throws and leaves pointers, capacity, row count and the live-bytes counter as they were; that moving empties the source; that drop and
release may be repeated; that no owner can be copied; and that the counter is zero when everything is gone.  The content-preserving regrow
(DevMem::regrow, DevKeep::ensure) goes 5 -> 12 -> 40 elements of 8 bytes: the prefix kept bit for bit, with zero-fill every other byte zero,
need <= cap a no-op that keeps the pointer, a failing allocation leaving pointer, capacity and counter as they were.  The capacity rule
(grown_cap) is checked against a copy of the loop it replaced, and PinnedMem for growth, grow-only, moves and no copies."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")

PROGRAM = r"""
#define MVS_DEV_MEM_HOST
#include "dev_mem.h"
#include <cstdio>
#include <type_traits>
#include <vector>
using namespace mvs;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static_assert(!std::is_copy_constructible<DevMem>::value && !std::is_copy_assignable<DevMem>::value, "DevMem copies");
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf copies");
static_assert(!std::is_copy_constructible<DevBlock<int>>::value && !std::is_copy_assignable<DevBlock<int>>::value, "DevBlock copies");
static_assert(!std::is_copy_constructible<DevRowStore>::value && !std::is_copy_assignable<DevRowStore>::value, "DevRowStore copies");
static_assert(!std::is_copy_constructible<DevKeep<int64_t>>::value && !std::is_copy_assignable<DevKeep<int64_t>>::value, "DevKeep copies");
static_assert(!std::is_copy_constructible<PinnedMem>::value && !std::is_copy_assignable<PinnedMem>::value, "PinnedMem copies");
static_assert(std::is_nothrow_move_constructible<PinnedMem>::value && std::is_nothrow_move_assignable<PinnedMem>::value, "PinnedMem moves");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBlock<int>>::value, "owners move");

constexpr size_t ROW = 8, SIDE = 4;
constexpr int64_t PAD = 3;
static unsigned char row_byte(int64_t r, size_t b) { return (unsigned char)(1 + (r * 31 + (int64_t)b * 7) % 251); }
static unsigned char side_byte(int64_t r, size_t b) { return (unsigned char)(1 + (r * 17 + (int64_t)b * 5) % 241); }
// "convert" rows [s.n, upto): what an ensure_*_rows launch does to the store
static void convert(DevRowStore &s, int64_t upto) {
	for (int64_t r = s.n; r < upto; ++r) {
		for (size_t b = 0; b < ROW; ++b)
			((unsigned char *)s.rows.p)[r * ROW + b] = row_byte(r, b);
		if (s.side_bytes)
			for (size_t b = 0; b < SIDE; ++b)
				((unsigned char *)s.side.p)[r * SIDE + b] = side_byte(r, b);
	}
	s.n = upto;
}
static void check_contents(const DevRowStore &s, const char *when) {
	CHECK(s.rows.cap == (size_t)(s.cap + PAD) * ROW, "%s: %zu row bytes for %lld + %lld rows", when, s.rows.cap, (long long)s.cap, (long long)PAD);
	CHECK(s.side.cap == (s.side_bytes ? (size_t)(s.cap + PAD) * SIDE : 0), "%s: %zu side bytes", when, s.side.cap);
	CHECK((s.side.p != nullptr) == (s.side_bytes != 0), "%s: side array", when);
	for (int64_t r = 0; r < s.cap + PAD; ++r) {
		for (size_t b = 0; b < ROW; ++b) {
			const unsigned char want = r < s.n ? row_byte(r, b) : 0, got = ((const unsigned char *)s.rows.p)[r * ROW + b];
			CHECK(got == want, "%s: row %lld byte %zu is %u, not %u", when, (long long)r, b, got, want);
		}
		if (s.side_bytes)
			for (size_t b = 0; b < SIDE; ++b) {
				const unsigned char want = r < s.n ? side_byte(r, b) : 0, got = ((const unsigned char *)s.side.p)[r * SIDE + b];
				CHECK(got == want, "%s: side %lld byte %zu is %u, not %u", when, (long long)r, b, got, want);
			}
	}
}
static int64_t store_bytes(const DevRowStore &s) { return (int64_t)(s.rows.cap + s.side.cap); }

static void row_store(bool with_side) {
	const int64_t base = g_dev_bytes_live.load();
	{
		DevRowStore s(ROW, with_side ? SIDE : 0, PAD);
		s.grow(5, nullptr);
		CHECK(s.cap == 5 && s.n == 0, "first growth: cap %lld n %lld", (long long)s.cap, (long long)s.n);
		check_contents(s, "fresh");
		convert(s, 5);
		check_contents(s, "5 converted");
		CHECK(g_dev_bytes_live.load() == base + store_bytes(s), "counter after the first growth");
		s.grow(4, nullptr); // (no shrinking, nothing moves)
		CHECK(s.cap == 5 && s.n == 5, "grow-only");
		s.grow(12, nullptr);
		CHECK(s.cap == 12 && s.n == 5, "second growth: cap %lld n %lld", (long long)s.cap, (long long)s.n);
		check_contents(s, "grown to 12");
		CHECK(g_dev_bytes_live.load() == base + store_bytes(s), "counter after the second growth (the old pair is gone)");
		convert(s, 9); // (a partly converted store grows too)
		// an allocation fails: the first, then (with a side array) the second
		for (int which = 1; which <= (with_side ? 2 : 1); ++which) {
			void *const rp = s.rows.p, *const sp = s.side.p;
			const int64_t live = g_dev_bytes_live.load();
			bool threw = false;
			g_dev_alloc_fail_at = which;
			try {
				s.grow(40, nullptr);
			} catch (const std::bad_alloc &) {
				threw = true;
			}
			g_dev_alloc_fail_at = 0;
			CHECK(threw, "allocation %d fails: grow must throw", which);
			CHECK(s.rows.p == rp && s.side.p == sp && s.cap == 12 && s.n == 9, "allocation %d fails: the store changed", which);
			CHECK(g_dev_bytes_live.load() == live, "allocation %d fails: the counter moved by %lld", which, (long long)(g_dev_bytes_live.load() - live));
			check_contents(s, "after a failed growth");
		}
		s.grow(40, nullptr);
		CHECK(s.cap == 40 && s.n == 9, "third growth");
		check_contents(s, "grown to 40");
		convert(s, 40);
		check_contents(s, "full");
		// moves empty the source
		DevRowStore t(std::move(s));
		CHECK(!s.rows.p && !s.side.p && s.rows.cap == 0 && s.side.cap == 0 && s.cap == 0 && s.n == 0, "move construction leaves the source holding something");
		CHECK(t.cap == 40 && t.n == 40, "move construction");
		check_contents(t, "moved");
		s.grow(6, nullptr); // (the emptied source is a usable store of the same shape)
		convert(s, 6);
		check_contents(s, "the source, built again");
		s = std::move(t); // (what s held is freed)
		CHECK(!t.rows.p && !t.side.p && t.cap == 0 && t.n == 0, "move assignment leaves the source holding something");
		CHECK(s.cap == 40 && s.n == 40, "move assignment");
		check_contents(s, "moved back");
		t = std::move(s);
		CHECK(g_dev_bytes_live.load() == base + store_bytes(t), "counter after the moves");
		t.drop();
		CHECK(!t.rows.p && !t.side.p && t.cap == 0 && t.n == 0 && t.row_bytes == ROW && t.pad == PAD, "drop");
		t.drop();
		CHECK(g_dev_bytes_live.load() == base, "counter after drop");
		t.grow(7, nullptr); // (rebuilt after a drop)
		convert(t, 6);
		check_contents(t, "rebuilt");
	}
	CHECK(g_dev_bytes_live.load() == base, "counter after the store's destructor");
}

// ---- the content-preserving regrow: elements of 8 bytes, 5 -> 12 -> 40
static uint64_t elem(size_t i) { return 0x9E3779B97F4A7C15ull * (i + 1); }
static void check_regrown(const DevMem &m, size_t cap_elems, size_t kept, bool zero, const char *when) {
	CHECK(m.p && m.cap == cap_elems * 8, "%s: capacity %zu bytes, not %zu", when, m.cap, cap_elems * 8);
	for (size_t i = 0; i < kept; ++i)
		CHECK(((const uint64_t *)m.p)[i] == elem(i), "%s: element %zu of the prefix changed", when, i);
	if (zero)
		for (size_t b = kept * 8; b < m.cap; ++b)
			CHECK(((const unsigned char *)m.p)[b] == 0, "%s: byte %zu beyond the prefix is not zero", when, b);
}
static void regrow(bool zero) {
	const int64_t base = g_dev_bytes_live.load();
	{
		DevMem m;
		m.regrow(5 * 8, 0, zero, nullptr);
		check_regrown(m, 5, 0, zero, "first regrow");
		for (size_t i = 0; i < 5; ++i)
			((uint64_t *)m.p)[i] = elem(i);
		void *p = m.p;
		m.regrow(4 * 8, 4 * 8, zero, nullptr);
		m.regrow(5 * 8, 5 * 8, zero, nullptr);
		CHECK(m.p == p && m.cap == 40, "need <= cap moved the allocation");
		m.regrow(12 * 8, 5 * 8, zero, nullptr);
		check_regrown(m, 12, 5, zero, "5 -> 12");
		CHECK(g_dev_bytes_live.load() == base + 96, "counter after 5 -> 12 (the old allocation is gone): %lld", (long long)(g_dev_bytes_live.load() - base));
		for (size_t i = 5; i < 12; ++i)
			((uint64_t *)m.p)[i] = elem(i);
		p = m.p;
		bool threw = false;
		g_dev_alloc_fail_at = 1;
		try {
			m.regrow(40 * 8, 12 * 8, zero, nullptr);
		} catch (const std::bad_alloc &) {
			threw = true;
		}
		g_dev_alloc_fail_at = 0;
		CHECK(threw, "a failing allocation: regrow must throw");
		CHECK(m.p == p && m.cap == 96 && g_dev_bytes_live.load() == base + 96, "a failing allocation changed pointer, capacity or counter");
		check_regrown(m, 12, 12, false, "after a failed regrow");
		m.regrow(40 * 8, 12 * 8, zero, nullptr);
		check_regrown(m, 40, 12, zero, "12 -> 40");
		CHECK(g_dev_bytes_live.load() == base + 320, "counter after 12 -> 40");
	}
	CHECK(g_dev_bytes_live.load() == base, "counter after the regrown allocation's destructor");
}
// (the loop every store carried before grown_cap)
template <class N>
static N old_rule(N cap, N need) {
	N nc = cap ? cap : 4096;
	while (nc < need)
		nc = nc + nc / 2 + 4096;
	return nc;
}

int main() {
	row_store(true);
	row_store(false);
	regrow(true);
	regrow(false);
	{ // the capacity rule, in the caller's units
		CHECK(grown_cap<int64_t>(0, 1) == 4096, "from 0 a need of 1: %lld", (long long)grown_cap<int64_t>(0, 1));
		CHECK(grown_cap<size_t>(4096, 4097) == 10240, "from 4096 a need of 4097: %zu", grown_cap<size_t>(4096, 4097));
		CHECK(grown_cap<int64_t>(0, 30000) == old_rule<int64_t>(0, 30000) && grown_cap<int64_t>(0, 30000) == 33280, "from 0 a need of 30000: %lld",
		      (long long)grown_cap<int64_t>(0, 30000));
		for (int64_t start : {0, 4096, 10240})
			for (int64_t need = 1; need <= 40000; need += 997) {
				CHECK(grown_cap<int64_t>(start, need) == old_rule<int64_t>(start, need), "rows: start %lld need %lld", (long long)start, (long long)need);
				CHECK(grown_cap<size_t>((size_t)start, (size_t)need) == old_rule<size_t>((size_t)start, (size_t)need), "bytes: start %lld need %lld",
				      (long long)start, (long long)need);
			}
	}
	{ // DevKeep: the rule in elements over the regrow (5 -> 12 -> 40 elements asked for; 4096 and 10240 held)
		DevKeep<int64_t> a;
		a.ensure(0, 0, nullptr);
		CHECK(!a.p && a.count() == 0, "ensure(0) allocated");
		a.ensure(5, 0, nullptr, true);
		CHECK(a.count() == 4096 && a.cap == 4096 * 8 && a.get() == (int64_t *)a.p, "ensure(5): %zu elements", a.count());
		for (size_t i = 0; i < 4096; ++i)
			a.get()[i] = (int64_t)elem(i);
		int64_t *const p = a.get();
		a.ensure(12, 5, nullptr);
		a.ensure(4096, 12, nullptr);
		CHECK(a.get() == p && a.count() == 4096, "need <= count moved the array");
		a.ensure(4097, 4096, nullptr, true);
		CHECK(a.count() == 10240 && g_dev_bytes_live.load() == 10240 * 8, "ensure(4097): %zu elements", a.count());
		check_regrown(a, 10240, 4096, true, "4096 -> 10240 elements");
		DevKeep<int64_t> b(std::move(a));
		CHECK(!a.p && a.count() == 0 && b.count() == 10240, "DevKeep move construction");
		b.release();
		b.release();
	}
	{ // PinnedMem: grow-only, 25 % + 256 bytes of slack, contents not kept
		PinnedMem h;
		CHECK(!h.p && h.cap == 0, "an empty pinned owner");
		void *p = h.reserve(100);
		CHECK(p && p == h.p && h.cap == 100 + 25 + 256, "reserve(100): %zu", h.cap);
		memset(h.p, 0xAB, h.cap);
		CHECK(h.reserve(64) == p && h.reserve(381) == p && h.cap == 381, "a smaller reserve keeps the pointer");
		h.reserve(1000, true);
		CHECK(h.p && h.cap == 1000 + 250 + 256, "reserve(1000): %zu", h.cap);
		memset(h.p, 0xCD, h.cap);
		p = h.p;
		PinnedMem g(std::move(h));
		CHECK(!h.p && h.cap == 0 && g.p == p && g.cap == 1506, "PinnedMem move construction");
		PinnedMem f;
		f.reserve(10);
		f = std::move(g); // (what f held is freed)
		CHECK(!g.p && g.cap == 0 && f.p == p && f.cap == 1506, "PinnedMem move assignment");
		f.release();
		f.release();
		CHECK(!f.p && f.cap == 0, "release");
		f.reserve(8); // (usable again; freed by the destructor)
	}
	{ // DevBuf: grow-only, 25 % + 256 bytes of slack, contents not kept
		DevBuf b;
		b.reserve(100);
		CHECK(b.p && b.cap == 100 + 25 + 256, "reserve(100): %zu", b.cap);
		void *p = b.p;
		b.reserve(300);
		CHECK(b.p == p && b.cap == 381, "a smaller request keeps the buffer");
		b.reserve(1000);
		CHECK(b.cap == 1000 + 250 + 256 && g_dev_bytes_live.load() == 1506, "reserve(1000): %zu, live %lld", b.cap, (long long)g_dev_bytes_live.load());
		DevBuf c(std::move(b));
		CHECK(!b.p && b.cap == 0 && c.cap == 1506, "DevBuf move construction");
		DevBuf e;
		e.reserve(10);
		e = std::move(c); // (what e held is freed)
		CHECK(!c.p && c.cap == 0 && e.cap == 1506 && g_dev_bytes_live.load() == 1506, "DevBuf move assignment, live %lld", (long long)g_dev_bytes_live.load());
		g_dev_alloc_fail_at = 1;
		bool threw = false;
		try {
			e.reserve(5000);
		} catch (const std::bad_alloc &) {
			threw = true;
		}
		g_dev_alloc_fail_at = 0;
		CHECK(threw && !e.p && e.cap == 0 && g_dev_bytes_live.load() == 0, "a failed reserve leaves the buffer empty (as before: the old one goes first)");
		e.release();
		e.release();
	}
	{ // DevBlock: exact size, typed, replaced only by a block that exists
		DevBlock<int64_t> ids(5);
		CHECK(ids && ids.cap == 40 && ids.get() == (int64_t *)ids.p, "DevBlock(5)");
		for (int i = 0; i < 5; ++i)
			ids.get()[i] = 100 + i;
		int64_t *const before = ids.get();
		g_dev_alloc_fail_at = 1;
		bool threw = false;
		try {
			ids = DevBlock<int64_t>(9);
		} catch (const std::bad_alloc &) {
			threw = true;
		}
		g_dev_alloc_fail_at = 0;
		CHECK(threw && ids.get() == before && ids.get()[4] == 104 && g_dev_bytes_live.load() == 40, "a failed replacement leaves the block");
		std::vector<DevBlock<int64_t>> retired; // (FlatIndex::Retired holds moved-in owners in a vector)
		retired.push_back(std::move(ids));
		retired.emplace_back(3);
		CHECK(!ids && ids.cap == 0 && retired[0].get() == before && g_dev_bytes_live.load() == 64, "moved into a vector");
		retired.erase(retired.begin());
		CHECK(g_dev_bytes_live.load() == 24 && retired[0].cap == 24, "erased from a vector: live %lld", (long long)g_dev_bytes_live.load());
		ids.release();
		ids.release();
		DevBlock<float> none;
		CHECK(!none && none.get() == nullptr, "an empty block");
	}
	CHECK(g_dev_bytes_live.load() == 0, "live bytes at exit: %lld", (long long)g_dev_bytes_live.load());
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_owners_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "dev_mem_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "dev_mem_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
