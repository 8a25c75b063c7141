// kernels_setup.hip -- a body's set-up on the device (setup.hpp): the initial
// state and the material ids of an inner box as pure functions of a node's
// coordinates, a short list of areas and a short list of vectors or ids.  Both
// kernels only write.  A work item is one segment of one row of the fastest axis
// (64 nodes for the ids, 256 for the state); a wave takes items in a grid stride
// and its lanes consecutive nodes, so every store of a wave is one run of 512
// bytes (64 bytes of ids).  Row
// bases are 64-bit and wave-uniform, the lane's offset within its row 32-bit; every
// stride comes from Geo.
#include "setup.hpp"

#include <algorithm>

namespace gcmx {

namespace {

// Area::contains (host/task.hpp:62-110), every kind strict.  The expressions keep
// the host's association; this file has the one build without contraction.
__device__ __forceinline__ bool area_contains(const gcmx_area& A, double c0, double c1, double c2) {
	const double* p = A.p;
	switch (A.kind) {
	case GCMX_AREA_BOX:
		if (c0 <= p[0] || c0 >= p[3]) return false;
		if (c1 <= p[1] || c1 >= p[4]) return false;
		if (c2 <= p[2] || c2 >= p[5]) return false;
		return true;
	case GCMX_AREA_SPHERE: {
		const double dx = c0 - p[1], dy = c1 - p[2], dz = c2 - p[3];
		return __dsqrt_rn(dx * dx + dy * dy + dz * dz) < p[0];
	}
	case GCMX_AREA_CYLINDER: {
		const double b0 = c0 - p[1], b1 = c1 - p[2], b2 = c2 - p[3];
		const double e0 = c0 - p[4], e1 = c1 - p[5], e2 = c2 - p[6];
		const double pb = b0 * p[7] + b1 * p[8] + b2 * p[9];
		const double pe = e0 * p[7] + e1 * p[8] + e2 * p[9];
		if (pb * pe >= 0) return false;
		return (b0 * b0 + b1 * b1 + b2 * b2) - pb * pb < p[0] * p[0];
	}
	default: return true;  // GCMX_AREA_INFINITE (the call refused any other kind)
	}
}

// CubicGrid::coords for one axis: two roundings and an add.
__device__ __forceinline__ double coord(int start, int it, double h) { return (double)start * h + (double)it * h; }

// A work item's row (a, b) and first node.
struct SetupItem {
	int a, b, f;
};
__device__ __forceinline__ SetupItem setup_item(const SetupBox& bx, long long item, int lane) {
	const long long row = item / bx.nseg;
	const int seg = (int)(item - row * bx.nseg);
	const int a = (int)(row / bx.nb);
	return {a, (int)(row - (long long)a * bx.nb), seg * 64 + lane};
}

// The node's coordinates by dimension: roles A, B, F are x, y, z in 3-D; x, -, y
// in 2-D; -, -, x in 1-D.
__device__ __forceinline__ void setup_coords(const SetupBox& bx, const SetupItem& it, double& c0, double& c1,
                                             double& c2) {
	// selects, not stores into an indexed triple (which would live in scratch)
	const double xa = coord(bx.ga, it.a, bx.ha), xb = coord(bx.gb, it.b, bx.hb), xf = coord(bx.gf, it.f, bx.hf);
	c0 = bx.D >= 2 ? xa : xf;
	c1 = bx.D == 3 ? xb : bx.D == 2 ? xf : 0.0;
	c2 = bx.D == 3 ? xf : 0.0;
}

__device__ __forceinline__ void setup_tables(unsigned long long* lds, const unsigned long long* __restrict__ tab_d,
                                             int words) {
	for (int i = threadIdx.x; i < words; i += 256) lds[i] = tab_d[i];
	__syncthreads();
}

// Nodes a lane of k_setup_state takes per item, 64 apart: a wave's item is a run
// of 256 nodes of a row, and all its 4 * M stores are issued after the last
// contains.  Measured at 512^3, M = 9, two areas (profiles/setup/tune.txt): 1, 2
// and 4 nodes per lane take 1.91-2.11, 1.69-1.86 and 1.64-1.77 ms against the
// same bytes' fill at 1.43 ms; plain stores in place of the non-temporal ones
// change nothing beyond the spread between processes.
constexpr int kStateNodes = 4;

// InitialCondition::apply (buildHostState): v = 0.0, then v += vec[k] for every
// area k that holds the node, in list order.
template <int M>
__global__ __launch_bounds__(256) void k_setup_state(double* __restrict__ cur, long long cs, long long origin,
                                                     SetupBox bx, int n,
                                                     const unsigned long long* __restrict__ tab_d) {
	extern __shared__ unsigned long long lds[];
	setup_tables(lds, tab_d, n * (kAreaWords + M));
	const gcmx_area* areas = reinterpret_cast<const gcmx_area*>(lds);
	const double* vec = reinterpret_cast<const double*>(lds + (size_t)n * kAreaWords);
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const long long nwaves = (long long)gridDim.x * 4;
	for (long long item = (long long)blockIdx.x * 4 + w; item < bx.items; item += nwaves) {
		SetupItem it = setup_item(bx, item, lane);
		const int f0 = (it.f - lane) * kStateNodes + lane;  // the lane's first node of the run
		double* row = cur + (origin + (long long)(bx.a0 + it.a) * bx.sa + (long long)(bx.b0 + it.b) * bx.sb);
		double v[kStateNodes][M];
#pragma unroll
		for (int j = 0; j < kStateNodes; j++) {
			it.f = f0 + 64 * j;
			double c0, c1, c2;
			setup_coords(bx, it, c0, c1, c2);
#pragma unroll
			for (int c = 0; c < M; c++) v[j][c] = 0.0;
			for (int k = 0; k < n; k++) {
				const bool in = area_contains(areas[k], c0, c1, c2);
#pragma unroll
				for (int c = 0; c < M; c++) v[j][c] = in ? v[j][c] + vec[k * M + c] : v[j][c];
			}
		}
#pragma unroll
		for (int j = 0; j < kStateNodes; j++) {
			const int f = f0 + 64 * j;
			if (f >= bx.nf) continue;
			const unsigned off = (unsigned)(bx.f0 + f);
#pragma unroll
			for (int c = 0; c < M; c++) __builtin_nontemporal_store(v[j][c], row + c * cs + off);
		}
	}
}

// MaterialsCondition::apply (buildHostState): id_of[k] of the last area k that
// holds the node, 0 when none does.  CENSUS: no store; the ids that occur go
// into a per-wave mask in LDS (one lane per distinct id of the wave's 64 nodes
// sets the bit), and the block's mask into used_d with one atomic OR per word.
template <bool CENSUS>
__global__ __launch_bounds__(256) void k_setup_ids(uint8_t* __restrict__ mat, SetupBox bx, int n,
                                                   const unsigned long long* __restrict__ tab_d,
                                                   unsigned* __restrict__ used_d) {
	extern __shared__ unsigned long long lds[];
	__shared__ unsigned mask[4][kCensusWords];
	if (CENSUS && threadIdx.x < 4 * kCensusWords) mask[threadIdx.x / kCensusWords][threadIdx.x % kCensusWords] = 0u;
	setup_tables(lds, tab_d, n * kAreaWords + (n + 7) / 8);
	const gcmx_area* areas = reinterpret_cast<const gcmx_area*>(lds);
	const uint8_t* id_of = reinterpret_cast<const uint8_t*>(lds + (size_t)n * kAreaWords);
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const long long nwaves = (long long)gridDim.x * 4;
	for (long long item = (long long)blockIdx.x * 4 + w; item < bx.items; item += nwaves) {
		const SetupItem it = setup_item(bx, item, lane);
		const bool live = it.f < bx.nf;
		int id = 0;
		if (live) {
			double c0, c1, c2;
			setup_coords(bx, it, c0, c1, c2);
			for (int k = 0; k < n; k++)
				if (area_contains(areas[k], c0, c1, c2)) id = id_of[k];
		}
		if constexpr (CENSUS) {
			unsigned long long pending = __ballot(live);
			while (pending) {  // once per distinct id among the wave's nodes
				const int v = __shfl(id, __ffsll((long long)pending) - 1);
				if (lane == 0) mask[w][v >> 5] |= 1u << (v & 31);
				pending &= ~__ballot(live && id == v);
			}
		} else if (live) {
			uint8_t* row = mat + ((long long)(bx.a0 + it.a) * bx.ma + (long long)(bx.b0 + it.b) * bx.mb);
			row[(unsigned)(bx.f0 + it.f)] = (uint8_t)id;
		}
	}
	if constexpr (CENSUS) {
		__syncthreads();
		if (threadIdx.x < kCensusWords) {
			const int k = threadIdx.x;
			const unsigned m = mask[0][k] | mask[1][k] | mask[2][k] | mask[3][k];
			if (m) atomicOr(&used_d[k], m);
		}
	}
}

// Enough blocks to keep every CU's wave slots busy, few enough that a block's
// table load into LDS is shared by many items.
unsigned setup_blocks(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + 3) / 4, 2048)); }

}  // namespace

SetupBox make_setup_box(const Geo& g, const int mn[3], const int mx[3], const int start[3], const double h[3]) {
	SetupBox bx{};
	bx.D = g.D;
	const int F = g.D - 1;
	bx.f0 = mn[F];
	bx.nf = mx[F] - mn[F];
	bx.gf = start[F];
	bx.hf = h[F];
	bx.na = bx.nb = 1;
	bx.ha = bx.hb = 0.0;
	if (g.D >= 2) {
		bx.a0 = mn[0];
		bx.na = mx[0] - mn[0];
		bx.sa = g.stride[0];
		bx.ma = (long long)g.sizes[1] * g.sizes[2];
		bx.ga = start[0];
		bx.ha = h[0];
	}
	if (g.D == 3) {
		bx.b0 = mn[1];
		bx.nb = mx[1] - mn[1];
		bx.sb = g.stride[1];
		bx.mb = g.sizes[2];
		bx.gb = start[1];
		bx.hb = h[1];
	}
	bx.nseg = (bx.nf + 63) / 64;
	bx.items = (long long)bx.na * bx.nb * bx.nseg;
	return bx;
}

void launch_setup_state(double* cur, const Geo& g, const SetupBox& box, int n, const unsigned long long* tab_d,
                        hipStream_t st) {
	SetupBox bx = box;  // the state kernel's items: runs of 64 * kStateNodes nodes
	bx.nseg = (bx.nf + 64 * kStateNodes - 1) / (64 * kStateNodes);
	bx.items = (long long)bx.na * bx.nb * bx.nseg;
	const dim3 grid(setup_blocks(bx.items)), block(256);
	const size_t lds = (size_t)n * (kAreaWords + g.M) * 8;
	switch (g.M) {  // the PDE vectors there are: elastic 2, 5, 9; acoustic 2, 3, 4
	case 2: hipLaunchKernelGGL(k_setup_state<2>, grid, block, lds, st, cur, g.cs, g.origin, bx, n, tab_d); break;
	case 3: hipLaunchKernelGGL(k_setup_state<3>, grid, block, lds, st, cur, g.cs, g.origin, bx, n, tab_d); break;
	case 4: hipLaunchKernelGGL(k_setup_state<4>, grid, block, lds, st, cur, g.cs, g.origin, bx, n, tab_d); break;
	case 5: hipLaunchKernelGGL(k_setup_state<5>, grid, block, lds, st, cur, g.cs, g.origin, bx, n, tab_d); break;
	default: hipLaunchKernelGGL(k_setup_state<9>, grid, block, lds, st, cur, g.cs, g.origin, bx, n, tab_d); break;
	}
}

void launch_setup_ids(uint8_t* mat_d, const Geo& g, const SetupBox& bx, int n, const unsigned long long* tab_d,
                      unsigned* used_d, hipStream_t st) {
	(void)g;
	const dim3 grid(setup_blocks(bx.items)), block(256);
	const size_t lds = ((size_t)n * kAreaWords + (size_t)(n + 7) / 8) * 8;
	if (mat_d) {
		hipLaunchKernelGGL(k_setup_ids<false>, grid, block, lds, st, mat_d, bx, n, tab_d, used_d);
		return;
	}
	(void)hipMemsetAsync(used_d, 0, kCensusWords * sizeof(unsigned), st);
	hipLaunchKernelGGL(k_setup_ids<true>, grid, block, lds, st, mat_d, bx, n, tab_d, used_d);
}

}  // namespace gcmx
