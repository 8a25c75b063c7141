// receiver_check.cpp -- the point receivers' corner and weight rule
// (gcm_amd/csrc/observe.hpp, receiver_corners) without a GPU: a stand-alone
// program, built with the address and undefined-behaviour sanitizers by
// tests/test_recorder_cpu.py.  Prints "checked <n>, <f> failed" last.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../gcm_amd/csrc/observe.hpp"

namespace {

long checked = 0, failed = 0;

void expect(bool ok, const char* what, int dim, int k) {
	checked++;
	if (ok) return;
	failed++;
	std::printf("FAILED %s (dim %d, case %d)\n", what, dim, k);
}

// the rule of include/gcmx.h written out again, per corner
double weight_of(int dim, const double* t, int k) {
	double w = 0;
	for (int d = 0; d < dim; d++) {
		const int bit = (k >> (dim - 1 - d)) & 1;
		const double f = bit ? t[d] : (1.0 - t[d]);
		w = d == 0 ? f : w * f;
	}
	return w;
}

void check_accept(int dim, const int* sizes, const double* pos, const int* want_base, const double* want_t, int id) {
	int base[3] = {-7, -7, -7};
	double w[8];
	for (double& x : w) x = -1.0;
	expect(gcmx::receiver_corners(dim, sizes, pos, base, w), "accepted", dim, id);
	for (int d = 0; d < dim; d++) expect(base[d] == want_base[d], "base index", dim, id);
	for (int d = dim; d < 3; d++) expect(base[d] == 0, "base index past dim", dim, id);
	double sum = 0;
	for (int k = 0; k < (1 << dim); k++) {
		expect(w[k] == weight_of(dim, want_t, k), "weight", dim, id);
		expect(w[k] >= 0.0 && w[k] <= 1.0, "weight in [0, 1]", dim, id);
		sum += w[k];
	}
	expect(std::fabs(sum - 1.0) <= 8 * std::numeric_limits<double>::epsilon(), "weights sum to one", dim, id);
	for (int k = (1 << dim); k < 8; k++) expect(w[k] == -1.0, "weights past 2^dim untouched", dim, id);
	// every corner is an inner node
	for (int k = 0; k < (1 << dim); k++)
		for (int d = 0; d < dim; d++) {
			const int i = base[d] + gcmx::receiver_corner_bit(dim, k, d);
			expect(i >= 0 && i < sizes[d], "corner inside the inner nodes", dim, id);
		}
}

void check_refuse(int dim, const int* sizes, const double* pos, int id) {
	int base[3];
	double w[8];
	expect(!gcmx::receiver_corners(dim, sizes, pos, base, w), "refused", dim, id);
}

}  // namespace

int main() {
	const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
	for (int dim = 1; dim <= 3; dim++) {
		const int sizes[3] = {7, 2, 5};  // axis 1 has the smallest size a point recorder takes
		// the last axis runs fastest: corner 1 differs from corner 0 on axis dim - 1 only
		expect(gcmx::receiver_corner_bit(dim, 1, dim - 1) == 1, "corner order", dim, 0);
		for (int d = 0; d + 1 < dim; d++) expect(gcmx::receiver_corner_bit(dim, 1, d) == 0, "corner order", dim, 0);
		expect(gcmx::receiver_corner_bit(dim, 1 << (dim - 1), 0) == 1, "corner order", dim, 0);
		{  // on a node: t = 0, the whole weight on corner 0
			const double pos[3] = {3.0, 0.0, 2.0};
			const int base[3] = {3, 0, 2};
			const double t[3] = {0.0, 0.0, 0.0};
			check_accept(dim, sizes, pos, base, t, 1);
			int b[3];
			double w[8];
			gcmx::receiver_corners(dim, sizes, pos, b, w);
			expect(w[0] == 1.0, "node: corner 0 has weight one", dim, 1);
			for (int k = 1; k < (1 << dim); k++) expect(w[k] == 0.0, "node: the other corners have weight zero", dim, 1);
		}
		{  // the upper edge: base sizes - 2, t = 1, the whole weight on the last corner
			const double pos[3] = {6.0, 1.0, 4.0};
			const int base[3] = {5, 0, 3};
			const double t[3] = {1.0, 1.0, 1.0};
			check_accept(dim, sizes, pos, base, t, 2);
			int b[3];
			double w[8];
			gcmx::receiver_corners(dim, sizes, pos, b, w);
			expect(w[(1 << dim) - 1] == 1.0, "upper edge: the last corner has weight one", dim, 2);
		}
		{  // between nodes; sizes_d = 2 on axis 1
			const double pos[3] = {2.25, 0.625, 3.9};
			const int base[3] = {2, 0, 3};
			const double t[3] = {2.25 - 2.0, 0.625 - 0.0, 3.9 - 3.0};
			check_accept(dim, sizes, pos, base, t, 3);
		}
		{  // the lower edge and a position just below the upper one
			const double below = std::nextafter(6.0, 0.0);
			const double pos[3] = {below, 0.0, 0.0};
			const int base[3] = {5, 0, 0};
			const double t[3] = {below - 5.0, 0.0, 0.0};
			check_accept(dim, sizes, pos, base, t, 4);
		}
		// the refusals, on every axis of the dimension
		for (int d = 0; d < dim; d++) {
			const double bad[] = {nan, -inf, inf, -0.5, -1e-300, std::nextafter((double)(sizes[d] - 1), inf),
			                      (double)sizes[d], 1e300};
			int id = 10;
			for (double x : bad) {
				double pos[3] = {1.0, 0.5, 1.0};
				pos[d] = x;
				check_refuse(dim, sizes, pos, id++);
			}
			int one[3] = {7, 2, 5};
			one[d] = 1;  // sizes_d = 1: no pair of nodes to blend
			const double pos[3] = {0.0, 0.0, 0.0};
			check_refuse(dim, one, pos, 30 + d);
		}
		{  // -0.0 is zero: accepted, on node 0
			const double pos[3] = {-0.0, -0.0, -0.0};
			const int base[3] = {0, 0, 0};
			const double t[3] = {0.0, 0.0, 0.0};
			check_accept(dim, sizes, pos, base, t, 5);
		}
	}
	{  // a dimension outside 1..3
		const int sizes[3] = {4, 4, 4};
		const double pos[3] = {1, 1, 1};
		check_refuse(0, sizes, pos, 40);
		check_refuse(4, sizes, pos, 41);
	}
	std::printf("checked %ld, %ld failed\n", checked, failed);
	return failed ? 1 : 0;
}
