"""The layout rule of a query block of the d <= 128 scan (csrc/flat_collect.h collect_qblock_wave): a stand-alone C++ program, built here
with AddressSanitizer and UBSan and run as a process of its own (nothing is loaded into Python), checks for every batch size from 129 to
2 560 and for 10 000, for every query block and both stage sizes (four row tiles on the int8 store, two on bf16), that every live (tile
column, row tile of a stage) job belongs to exactly one wave, that no wave has more than four columns, that a wave runs nested prefixes
of its slots, that the jobs per wave and stage are T on the int8 store (T live columns; sixteen at T = 15, which no four-slot layout does
in fewer: see the rule's comment), that every live query has exactly one table slot in every wave that works on it and none elsewhere,
and that full blocks -- and every block of the bf16 store -- keep the layout of four consecutive columns per wave."""

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
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 50) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } } while (0)
static void check(int nq, int S) {
	const int nqb = (nq + 511) / 512;
	for (int qb = 0; qb < nqb; ++qb) {
		const int live = nq - qb * 512 < 512 ? nq - qb * 512 : 512;
		const int T = (live + 31) / 32;
		CHECK(collect_qblock_cols(nq, qb) == T, "nq %d qb %d: T %d, rule says %d", nq, qb, T, collect_qblock_cols(nq, qb));
		const int Tl = T == 15 || S != 4 ? 16 : T; // (T = 15 and the bf16 store run the full layout, dead columns included)
		int done[16][4] = {};  // jobs: (tile column, row tile of a stage) -> waves that run it
		int holders[16] = {};  // waves with a table slot for the column
		for (int w = 0; w < 4; ++w) {
			const unsigned word = collect_qblock_wave(nq, qb, S, w);
			int jobs = 0, used = 0, seen = 0;
			for (int s = 0; s < S; ++s) {
				const int n = collect_qblock_ncols(word, s);
				CHECK(n >= 0 && n <= 4, "nq %d qb %d S %d wave %d: %d columns on row tile %d", nq, qb, S, w, n, s);
				jobs += n;
				used = n > used ? n : used;
				for (int t = 0; t < n && t < 4; ++t)
					++done[collect_qblock_slot_col(word, t)][s];
			}
			// the slots: the used ones name distinct live columns, the free ones a column without a live query
			for (int t = 0; t < 4; ++t) {
				const int col = collect_qblock_slot_col(word, t);
				if (t < used) {
					CHECK(col < Tl, "nq %d qb %d S %d wave %d: slot %d runs dead column %d", nq, qb, S, w, t, col);
					CHECK(!((seen >> col) & 1), "nq %d qb %d S %d wave %d: column %d in two slots", nq, qb, S, w, col);
					seen |= 1 << col;
					++holders[col];
				} else {
					CHECK(col >= Tl, "nq %d qb %d S %d wave %d: free slot %d names live column %d", nq, qb, S, w, t, col);
				}
			}
			if (T == 16 || T == 15 || S != 4) { // today's layout (the bf16 store keeps it for every block)
				for (int t = 0; t < 4; ++t)
					CHECK(collect_qblock_slot_col(word, t) == 4 * w + t, "nq %d qb %d S %d wave %d: full block, slot %d = column %d", nq, qb, S, w, t, collect_qblock_slot_col(word, t));
				CHECK(jobs == 4 * S, "nq %d qb %d S %d wave %d: full block, %d jobs", nq, qb, S, w, jobs);
			} else {
				CHECK(jobs == T, "nq %d qb %d wave %d: %d jobs per stage, T = %d", nq, qb, w, jobs, T);
			}
		}
		for (int col = 0; col < 16; ++col) {
			for (int s = 0; s < S; ++s)
				CHECK(done[col][s] == (col < Tl ? 1 : 0), "nq %d qb %d S %d: job (column %d, row tile %d) done %d times", nq, qb, S, col, s, done[col][s]);
			// (a wave that works on a column holds it in exactly one slot -- `seen` above -- and a wave that holds it works on it)
			CHECK(col < Tl ? holders[col] >= 1 : holders[col] == 0, "nq %d qb %d S %d: column %d has %d holders", nq, qb, S, col, holders[col]);
		}
	}
}
int main() {
	for (int S = 4; S >= 2; S -= 2) {
		for (int nq = 129; nq <= 2560; ++nq)
			check(nq, S);
		check(10000, S);
	}
	// the headline's last block on the int8 store: waves own {0,1} {2,3} {4,5} {6,7}, share column 8, nine jobs each
	for (int w = 0; w < 4; ++w) {
		const unsigned word = collect_qblock_wave(10000, 19, 4, w);
		CHECK(collect_qblock_slot_col(word, 0) == 2 * w && collect_qblock_slot_col(word, 1) == 2 * w + 1 && collect_qblock_slot_col(word, 2) == 8,
		      "headline, wave %d: columns %d %d %d", w, collect_qblock_slot_col(word, 0), collect_qblock_slot_col(word, 1), collect_qblock_slot_col(word, 2));
		for (int s = 0; s < 4; ++s)
			CHECK(collect_qblock_ncols(word, s) == (s == w ? 3 : 2), "headline, wave %d row tile %d: %d columns", w, s, collect_qblock_ncols(word, s));
	}
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_layout_rule_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "layout_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
