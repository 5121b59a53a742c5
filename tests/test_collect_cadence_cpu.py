"""The pacing of the d <= 128 scan's bound upkeep (csrc/flat_collect.h collect_upkeep_periods, collect_seen_rows, collect_upkeep_due): a
stand-alone C++ program, built here with AddressSanitizer and UBSan and run as a process of its own (nothing is loaded into Python), walks
the range-major item order of the plans of N = 262 221, 1 M, 1.25 M and 10 M rows (int8 store: stages of 128 rows, 768 workgroups; 1, 2
and 20 query blocks) and checks that both periods are powers of two between their floor and ceiling, that they never decrease along the
order, that the first round of items has the floor, that the rows an item takes as seen are rows of ranges handed out before it and at
least a round of the workgroups back, and that no item derives more often than its stages allow: an item of one stage at most once."""

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
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
int main() {
	const int64_t ns[] = {262221, 1000000, 1250000, 10000000};
	const int nqbs[] = {1, 2, 20};
	const int stage = 128, slots = 768;
	const int d_floor = CL_UPKEEP_FLOOR_ROWS / stage, d_ceil = CL_UPKEEP_CEIL_ROWS / stage;
	const int f_floor = CL_UPKEEP_FETCH_FLOOR_ROWS / stage, f_ceil = d_ceil / CL_UPKEEP_FETCH_DIV > f_floor ? d_ceil / CL_UPKEEP_FETCH_DIV : f_floor;
	CHECK(pow2(d_floor) && pow2(d_ceil) && pow2(f_floor) && d_floor <= d_ceil, "floor %d and ceiling %d stages", d_floor, d_ceil);
	for (int64_t n : ns)
		for (int nqb : nqbs) {
			const CollectSched s = collect_plan_levels(n, stage, nqb, slots);
			const std::vector<int64_t> b = collect_plan_ranges(n, stage, nqb, slots);
			const int grid = (int64_t)s.nranges * nqb < slots ? s.nranges * nqb : slots; // the launch: a workgroup per slot, or per item
			const int at_work = (grid + nqb - 1) / nqb;
			CollectUpkeep prev = {0, 0};
			int64_t prev_seen = -1;
			bool reached_ceiling = false;
			for (int r = 0; r < s.nranges; ++r) { // (the order is range-major: the items of a range share its periods)
				CHECK(collect_range_begin(&s, r) == b[r], "n %lld: range %d begins at %lld, the plan says %lld", (long long)n, r, (long long)collect_range_begin(&s, r), (long long)b[r]);
				const int64_t seen = collect_seen_rows(&s, r, nqb, grid);
				CHECK(seen >= prev_seen && seen <= b[r], "n %lld nqb %d: range %d sees %lld rows (before it: %lld, its first row %lld)", (long long)n, nqb, r, (long long)seen, (long long)prev_seen, (long long)b[r]);
				CHECK(r > at_work ? seen == b[r - at_work] : seen == 0, "n %lld nqb %d: range %d sees %lld rows, %d ranges are at work", (long long)n, nqb, r, (long long)seen, at_work);
				const CollectUpkeep up = collect_upkeep_periods(seen, stage);
				CHECK(pow2(up.derive) && up.derive >= d_floor && up.derive <= d_ceil, "n %lld range %d: derivation period %d", (long long)n, r, up.derive);
				CHECK(pow2(up.fetch) && up.fetch >= f_floor && up.fetch <= f_ceil && up.fetch <= up.derive, "n %lld range %d: fetch period %d", (long long)n, r, up.fetch);
				CHECK(up.derive >= prev.derive && up.fetch >= prev.fetch, "n %lld nqb %d range %d: periods %d / %d after %d / %d", (long long)n, nqb, r, up.derive, up.fetch, prev.derive, prev.fetch);
				if (r <= at_work)
					CHECK(up.derive == d_floor && up.fetch == f_floor, "n %lld nqb %d: range %d of the first round has periods %d / %d", (long long)n, nqb, r, up.derive, up.fetch);
				// the period doubles no sooner than the rows seen allow: a derivation per 1 / CL_UPKEEP_SHARE of them
				CHECK(up.derive == d_floor || (int64_t)up.derive * stage * CL_UPKEEP_SHARE <= seen, "n %lld range %d: period %d at %lld rows", (long long)n, r, up.derive, (long long)seen);
				CHECK(up.derive == d_ceil || (int64_t)2 * up.derive * stage * CL_UPKEEP_SHARE > seen, "n %lld range %d: period %d at %lld rows is short", (long long)n, r, up.derive, (long long)seen);
				reached_ceiling |= up.derive == d_ceil;
				const int stages = (int)((b[r + 1] - b[r] + stage - 1) / stage);
				int due = 0;
				for (int u = 0; u < stages; ++u)
					due += collect_upkeep_due(u, r, up.derive) ? 1 : 0;
				CHECK(due <= (stages + up.derive - 1) / up.derive, "n %lld range %d: %d derivations in %d stages at period %d", (long long)n, r, due, stages, up.derive);
				if (stages == 1)
					CHECK(due <= 1, "n %lld range %d: a single stage derives %d times", (long long)n, r, due);
				prev = up;
				prev_seen = seen;
			}
			if (n >= 1000000 && nqb == 20) // (39 ranges at work, half a million rows behind the grid: the ceiling; few query blocks: one round)
				CHECK(reached_ceiling, "n %lld nqb %d: the period never reaches its ceiling", (long long)n, nqb);
		}
	// the rule on its own: the floor below CL_UPKEEP_SHARE floor periods of rows, one doubling per doubling of the rows, the ceiling held
	CHECK(collect_upkeep_periods(0, stage).derive == d_floor && collect_upkeep_periods(2 * CL_UPKEEP_FLOOR_ROWS * CL_UPKEEP_SHARE - 1, stage).derive == d_floor, "floor");
	CHECK(collect_upkeep_periods(2 * CL_UPKEEP_FLOOR_ROWS * CL_UPKEEP_SHARE, stage).derive == 2 * d_floor, "first doubling");
	CHECK(collect_upkeep_periods((long long)1 << 40, stage).derive == d_ceil && collect_upkeep_periods((long long)1 << 40, 64).derive == CL_UPKEEP_CEIL_ROWS / 64, "ceiling");
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_upkeep_periods_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "cadence_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "cadence_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
