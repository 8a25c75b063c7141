// snapshot_strided_check.cpp -- the GPU-free strided VtkSnapshotter writer
// (gcm_amd/host/snapshot.cpp) as a stand-alone program: tests/
// test_snapshot_strided_cpu.py builds it together with snapshot.cpp under
// -fsanitize=address,undefined and runs it; needs no GPU.  Prints "ok <checks>"
// as its last line, or the first failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../gcm_amd/host/acoustic_model.hpp"
#include "../gcm_amd/host/snapshot.hpp"

using namespace gcm;
using namespace gcm::cubic;

static int checks = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		checks++;                                                          \
		if (!(cond)) {                                                     \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			std::exit(1);                                                  \
		}                                                                  \
	} while (0)

static std::string slurp(const std::string& name) {
	std::ifstream f(name, std::ios::binary);
	return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

template <int D>
static void body(const std::string& dir, std::array<int, D> sizes, std::array<int, D> start, Models::T model,
                 const std::vector<PhysicalQuantities::T>& quantities, VtkSelection<D> sel) {
	const int bs = 2, M = pdeSizeOf(model, D);
	std::array<real, D> h;
	size_t all = 1;
	long long im[3] = {0, 0, 0};
	for (int i = D - 1; i >= 0; i--) {
		h[i] = 0.25 + 0.5 * i;
		im[i] = (long long)all;
		all *= (size_t)(sizes[i] + 2 * bs);
	}
	std::vector<real> pde(all * M);
	std::vector<uint8_t> ids(all);
	for (size_t p = 0; p < all; p++) {
		ids[p] = (uint8_t)(p % 3);
		for (int c = 0; c < M; c++) pde[p * M + c] = (real)((p * 31 + c * 7) % 1021) / 8.0 - 60.0;
	}
	const std::vector<int> numbers = {5, 9, 2};
	const std::string tag = dir + "/d" + std::to_string(D);

	// the whole body at stride 1 is the existing writer's file byte for byte
	VtkSelection<D> whole;
	for (int i = 0; i < D; i++) {
		whole.lo[i] = 0;
		whole.hi[i] = sizes[i];
		whole.stride[i] = 1;
	}
	writeVtkSnapshot<D>(tag + "_old.vts", sizes, start, h, bs, pde.data(), ids.data(), numbers, quantities, model);
	writeVtkSnapshot<D>(tag + "_whole.vts", sizes, start, h, bs, pde.data(), ids.data(), numbers, quantities, model,
	                    whole);
	CHECK(!slurp(tag + "_old.vts").empty());
	CHECK(slurp(tag + "_old.vts") == slurp(tag + "_whole.vts"));

	// the arrays of a selection are the full-resolution arrays at the selected nodes
	VtsArray fv, sv;
	std::vector<VtsArray> fq, sq;
	vtkLayerArrays<D>(sizes, bs, pde.data(), quantities, model, fv, fq);
	vtkLayerArrays<D>(sizes, bs, pde.data(), quantities, model, sel, sv, sq);
	int full[3] = {1, 1, 1}, n[3] = {1, 1, 1}, lo[3] = {0, 0, 0}, st[3] = {1, 1, 1};
	for (int i = 0; i < D; i++) {
		full[i] = sizes[i];
		n[i] = sel.points(i);
		lo[i] = sel.lo[i];
		st[i] = sel.stride[i];
		CHECK(lo[i] + (n[i] - 1) * st[i] < sel.hi[i] && lo[i] + n[i] * st[i] >= sel.hi[i]);
	}
	CHECK(sv.values.size() == 3 * sel.points() && sq.size() == quantities.size());
	size_t p = 0;
	for (int z = 0; z < n[2]; z++)
		for (int y = 0; y < n[1]; y++)
			for (int x = 0; x < n[0]; x++, p++) {
				const size_t f = ((size_t)(lo[2] + z * st[2]) * full[1] + (lo[1] + y * st[1])) * full[0] + lo[0] + x * st[0];
				for (int c = 0; c < 3; c++) CHECK(sv.values[3 * p + c] == fv.values[3 * f + c]);
				for (size_t k = 0; k < sq.size(); k++) CHECK(sq[k].values[p] == fq[k].values[f]);
			}
	writeVtkSnapshot<D>(tag + "_sel.vts", sizes, start, h, bs, pde.data(), ids.data(), numbers, quantities, model, sel);
	const std::string file = slurp(tag + "_sel.vts");
	const std::string ext = "WholeExtent=\"0 " + std::to_string(n[0] - 1) + " 0 " + std::to_string(n[1] - 1) + " 0 " +
	                        std::to_string(n[2] - 1) + "\"";
	CHECK(file.find(ext) != std::string::npos);
	CHECK(file.size() < slurp(tag + "_old.vts").size() || sel.points() == whole.points());
	(void)im;

	// refusals of the writer
	VtkSelection<D> bad = sel;
	bad.stride[0] = 0;
	bool threw = false;
	try {
		vtkLayerArrays<D>(sizes, bs, pde.data(), quantities, model, bad, sv, sq);
	} catch (const std::exception&) {
		threw = true;
	}
	CHECK(threw);
	bad = sel;
	bad.hi[D - 1] = sizes[D - 1] + 1;
	threw = false;
	try {
		writeVtkSnapshot<D>(tag + "_bad.vts", sizes, start, h, bs, pde.data(), ids.data(), numbers, quantities, model,
		                    bad);
	} catch (const std::exception&) {
		threw = true;
	}
	CHECK(threw);
}

static void selections() {
	Task::VtkSnapshotter s;
	VtkSelection<3> sel;
	const std::array<int, 3> sizes = {10, 7, 64}, start = {0, 5, -3};
	CHECK(vtkSelectionOf<3>(s, sizes, start, sel));
	CHECK(sel.lo == (std::array<int, 3>{0, 0, 0}) && sel.hi == sizes && sel.stride == (std::array<int, 3>{1, 1, 1}));
	s.stride = {2, 3, 200};
	CHECK(vtkSelectionOf<3>(s, sizes, start, sel));
	CHECK(sel.points(0) == 5 && sel.points(1) == 3 && sel.points(2) == 1 && sel.points() == 15);
	s.hasBox = true;
	s.boxMin = {1, 2, -1000000000};
	s.boxMax = {9, 11, 2000000000};
	CHECK(vtkSelectionOf<3>(s, sizes, start, sel));
	CHECK(sel.lo == (std::array<int, 3>{1, 0, 0}) && sel.hi == (std::array<int, 3>{9, 6, 64}));
	s.boxMax = {9, 5, 10};  // ends where this body begins on y
	CHECK(!vtkSelectionOf<3>(s, sizes, start, sel));
	s.boxMin = {10, 2, 0};  // begins where this body ends on x
	s.boxMax = {20, 11, 10};
	CHECK(!vtkSelectionOf<3>(s, sizes, start, sel));
	s.hasBox = false;
	s.stride = {1, 0, 1};
	bool threw = false;
	try {
		vtkSelectionOf<3>(s, sizes, start, sel);
	} catch (const std::exception&) {
		threw = true;
	}
	CHECK(threw);
}

int main(int argc, char** argv) {
	const std::string dir = argc > 1 ? argv[1] : ".";
	typedef PhysicalQuantities::T Q;
	body<3>(dir, {7, 5, 9}, {0, 0, 0}, Models::T::ELASTIC, {Q::PRESSURE, Q::Vz, Q::Syz}, {{1, 0, 2}, {7, 5, 8}, {3, 2, 4}});
	body<3>(dir, {7, 5, 9}, {3, -2, 1}, Models::T::ELASTIC, {Q::PRESSURE}, {{0, 0, 0}, {7, 5, 9}, {8, 5, 100}});
	body<3>(dir, {4, 3, 5}, {0, 0, 0}, Models::T::ACOUSTIC, {Q::PRESSURE, Q::Vx}, {{0, 1, 0}, {4, 3, 5}, {1, 1, 2}});
	body<2>(dir, {9, 13}, {3, -2}, Models::T::ELASTIC, {Q::Sxy, Q::PRESSURE}, {{1, 1}, {9, 12}, {2, 5}});
	body<2>(dir, {6, 4}, {0, 0}, Models::T::ACOUSTIC, {Q::PRESSURE}, {{5, 3}, {6, 4}, {1, 1}});
	body<1>(dir, {40}, {7}, Models::T::ELASTIC, {Q::Vx, Q::PRESSURE}, {{3}, {38}, {7}});
	selections();
	std::printf("ok %d\n", checks);
	return 0;
}
