"""The range rule of the persistent d <= 128 scan (csrc/flat_collect.h collect_plan_ranges): a stand-alone C++ program, built here with
AddressSanitizer and UBSan and run as a process of its own (nothing is loaded into Python), checks over a grid of store sizes, query
blocks and both stage sizes that the ranges are contiguous and cover the rows exactly once, that every boundary but the end is a multiple
of the stage, that sizes never increase, that the body keeps the one-shot planner's split size, that the taper shrinks to its floor, that
the number of items stays bounded, and that every XCD queue has work once there are eight ranges."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")

PROGRAM = r"""
#define MVS_COLLECT_PLAN_ONLY
#include "flat_collect.h"
#include <cstdio>
#include <cstdlib>
using namespace mvs;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)
int main() {
	const int64_t ns[] = {1, 63, 64, 129, 7680, 262144, 262145, 1250000, 10000000, ((int64_t)1 << 31) + 5};
	const int64_t nqbs[] = {1, 3, 20, 61};
	const int64_t stages[] = {128, 64}; // int8 store (768 slots), bf16 store (512)
	for (int64_t stage : stages)
		for (int64_t n : ns)
			for (int64_t nqb : nqbs) {
				const int64_t slots = stage == 128 ? 768 : 512;
				const std::vector<int64_t> b = collect_plan_ranges(n, stage, nqb, slots);
				const CollectSched s = collect_plan_levels(n, stage, nqb, slots);
				const int64_t nr = (int64_t)b.size() - 1;
				CHECK(nr >= 1 && nr == s.nranges, "n %lld nqb %lld stage %lld: %lld ranges, plan says %d", (long long)n, (long long)nqb, (long long)stage, (long long)nr, s.nranges);
				CHECK(b.front() == 0 && b.back() == n, "n %lld: covers [%lld, %lld)", (long long)n, (long long)b.front(), (long long)b.back());
				CHECK(s.nlev >= 1 && s.nlev <= CL_SCHED_LEVELS, "n %lld: %d levels", (long long)n, s.nlev);
				int64_t prev = -1;
				for (int64_t r = 0; r < nr; ++r) {
					const int64_t len = b[r + 1] - b[r];
					CHECK(len > 0, "n %lld nqb %lld: range %lld is empty", (long long)n, (long long)nqb, (long long)r);
					CHECK(r + 1 == nr || b[r + 1] % stage == 0, "n %lld: boundary %lld not a multiple of the stage", (long long)n, (long long)b[r + 1]);
					CHECK(prev < 0 || len <= prev, "n %lld nqb %lld: range %lld grows (%lld after %lld)", (long long)n, (long long)nqb, (long long)r, (long long)len, (long long)prev);
					prev = len;
				}
				// the body: the one-shot planner's split -- at least 7 680 rows, at most 384 of them -- rounded up to whole stages
				const int64_t nbody = n / 7680 < 1 ? 1 : (n / 7680 > 384 ? 384 : n / 7680);
				const int64_t body = ((n + stage - 1) / stage + nbody - 1) / nbody * stage;
				CHECK(b[1] - b[0] <= body, "n %lld: first range %lld above the body size %lld", (long long)n, (long long)(b[1] - b[0]), (long long)body);
				if (n >= 4 * 7680 && (slots + nqb - 1) / nqb * CL_TAPER_ROUNDS * 2 < nbody) // (a body exists: the taper takes less than half)
					CHECK(b[1] - b[0] == body, "n %lld nqb %lld: body range %lld, expected %lld", (long long)n, (long long)nqb, (long long)(b[1] - b[0]), (long long)body);
				// the taper: from level to level the size halves (rounded up to a stage) and ends at the floor
				int64_t floor_rows = (512 + stage - 1) / stage * stage;
				if (floor_rows < (body / stage + 511) / 512 * stage)
					floor_rows = (body / stage + 511) / 512 * stage;
				for (int l = 1; l < s.nlev; ++l)
					CHECK(s.rows[l] < s.rows[l - 1] && s.rows[l] >= floor_rows && s.rows[l] % stage == 0, "n %lld: level %d of %d rows after %d", (long long)n, l, s.rows[l], s.rows[l - 1]);
				if (n > floor_rows)
					CHECK(s.rows[s.nlev - 1] == floor_rows, "n %lld nqb %lld: last level %d rows, floor %lld", (long long)n, (long long)nqb, s.rows[s.nlev - 1], (long long)floor_rows);
				// items: the body's, plus at most CL_TAPER_ROUNDS rounds of the slots per level (+ a range per level for rounding)
				const int64_t bound = (nbody + 1) * nqb + (int64_t)CL_SCHED_LEVELS * (CL_TAPER_ROUNDS * (slots + nqb) + 2 * nqb);
				CHECK(nr * nqb <= bound, "n %lld nqb %lld: %lld items, bound %lld", (long long)n, (long long)nqb, (long long)(nr * nqb), (long long)bound);
				CHECK(nr * nqb < ((int64_t)1 << 28), "n %lld: item numbers must fit 28 bits", (long long)n);
				// queues: range r -> queue r & 7; together they hold every item once, and none is empty from eight ranges on
				int64_t sum = 0;
				for (int x = 0; x < 8; ++x) {
					const int64_t c = collect_queue_items((int)nr, x, nqb);
					sum += c;
					CHECK(nr < 8 || c > 0, "n %lld: queue %d empty with %lld ranges", (long long)n, x, (long long)nr);
					CHECK(c == ((nr - x + 7) / 8) * nqb || nr <= x, "n %lld: queue %d holds %lld", (long long)n, x, (long long)c);
				}
				CHECK(sum == nr * nqb, "n %lld: queues hold %lld of %lld items", (long long)n, (long long)sum, (long long)(nr * nqb));
			}
	CHECK(collect_plan_ranges(0, 128, 1, 768).size() == 1, "an empty store has no range");
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_range_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "ranges_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ranges_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
