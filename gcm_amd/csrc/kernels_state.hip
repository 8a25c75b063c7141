// kernels_state.hip -- the exact fp64 state of a box, planes <-> AoS staging
// (state.hpp).  An HBM-bound transposition of 2 * M * 8 bytes per node.  Strides
// come from Geo, so padded layouts work; element offsets are formed in 64 bits.
#include "state.hpp"

#include <algorithm>

namespace gcmx {

namespace {

__device__ __forceinline__ double nt_load(const double* p) { return __builtin_nontemporal_load(p); }

constexpr int kTileNodes = 64;  // one wave's item: 64 consecutive nodes of one row

// The tile of one wave: the item's 64 * M doubles in AoS order (element
// e = node * M + component), each aligned group of 16 doubles rotated by r(j),
// j = e / 16:  slot(e) = (e & ~15) | ((e + r(j)) & 15).
//
// Banks (a double at index i covers dwords 2 i, 2 i + 1): ds_write_b64 is served
// in four groups of 16 consecutive lanes with the dword modulo 32, so a group's
// 16 indices must differ modulo 16; ds_read_b64 in two groups of 32 lanes with
// the dword modulo 64, so a group's 32 indices must differ modulo 32.
//   AoS side, lane l at e = l + 64 k: a group's elements fill whole 16-groups,
//     and a rotation permutes a 16-group in itself: conflict-free for any r.
//   Plane side, lane l at e = l M + c: for odd M, M is a unit modulo 16 and 32,
//     so r = 0 does.  M = 2: 16 lanes cover two 16-groups with the same even
//     residues, 32 lanes four; r(j) = j + (j >> 1) = 0, 1, 3, 4, ... gives the
//     pair (j, j + 1) opposite parities (write) and, per 32-half, the two
//     16-groups that share a half (j, j + 2) opposite parities (read).  M = 4:
//     16 lanes cover four 16-groups with residues 4 i + c, 32 lanes eight;
//     r(j) = j + (j >> 2) = 0, 1, 2, 3, 5, 6, 7, 8 is distinct modulo 4 over
//     (4 q .. 4 q + 3) (write) and over the four groups of either 32-half
//     (0, 2, 5, 7 and 1, 3, 6, 8) (read).
// DESIGN.md §3.6.2 has the arithmetic; no padding, 512 * M bytes per wave.
template <int M>
__device__ __forceinline__ int tile_slot(int e) {
	static_assert(M % 2 == 1 || M == 2 || M == 4, "no conflict-free rotation worked out for this M");
	if constexpr (M % 2 == 1) {
		return e;
	} else {
		const int j = e >> 4;
		const int r = M == 2 ? j + (j >> 1) : j + (j >> 2);
		return (e & ~15) | ((e + r) & 15);
	}
}

// What a wave needs of its item: wave-uniform, 64-bit bases.
struct StateItem {
	long long plane;  // element offset of the item's first node in a component plane
	long long stage;  // element offset of the item's first value in the staging
	int width;        // nodes of the item (< 64 in a row's last tile)
	bool live;
};

__device__ __forceinline__ StateItem state_item(const StateBox& bx, int row0, unsigned items, int M) {
	const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const unsigned item = blockIdx.x * 4u + (unsigned)w;
	StateItem it;
	it.live = item < items;
	const unsigned rl = item / (unsigned)bx.tf, t = item - rl * (unsigned)bx.tf;
	const int row = row0 + (int)rl;
	const int a = row / bx.nb, b = row - a * bx.nb;
	it.plane = bx.base + (long long)a * bx.sa + (long long)b * bx.sb + (long long)t * kTileNodes;
	it.stage = ((long long)rl * bx.nf + (long long)t * kTileNodes) * M;
	it.width = min(kTileNodes, bx.nf - (int)t * kTileNodes);
	return it;
}

// Block = four waves, each with an item and a tile of its own.  Planes side: M
// coalesced runs of 64 doubles, one per component; a lane past the item's last
// node reads that node again (a load without a branch; never stored).  Staging
// side: one contiguous run of width * M doubles, M instructions of 64
// consecutive doubles.  All M loads issue before the first LDS write waits.
template <int M>
__global__ __launch_bounds__(256) void k_state_pack(const double* __restrict__ cur, StateBox bx, int row0,
                                                    unsigned items, double* __restrict__ stage) {
	__shared__ double tile[4][kTileNodes * M];
	const int lane = threadIdx.x & 63;
	const StateItem it = state_item(bx, row0, items, M);
	double* tl = tile[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	if (it.live) {
		const double* src = cur + it.plane;
		const unsigned l = (unsigned)min(lane, it.width - 1);  // 32-bit lane offset on a uniform 64-bit base
		double v[M];
#pragma unroll
		for (int c = 0; c < M; c++) v[c] = nt_load(src + c * bx.cs + l);
#pragma unroll
		for (int c = 0; c < M; c++) tl[tile_slot<M>(lane * M + c)] = v[c];
	}
	__syncthreads();
	if (it.live) {
		double* dst = stage + it.stage;
		const int n = it.width * M;
		double o[M];  // every LDS read in flight before the first store waits
#pragma unroll
		for (int k = 0; k < M; k++) o[k] = tl[tile_slot<M>(lane + kTileNodes * k)];
#pragma unroll
		for (int k = 0; k < M; k++) {
			const int e = lane + kTileNodes * k;
			if (e < n) __builtin_nontemporal_store(o[k], dst + (unsigned)e);
		}
	}
}

// The reverse.  A staging element past the item's last one reads that one again
// (inside the chunk); a lane past the item's last node stores nothing.
template <int M>
__global__ __launch_bounds__(256) void k_state_unpack(double* __restrict__ cur, StateBox bx, int row0,
                                                      unsigned items, const double* __restrict__ stage) {
	__shared__ double tile[4][kTileNodes * M];
	const int lane = threadIdx.x & 63;
	const StateItem it = state_item(bx, row0, items, M);
	double* tl = tile[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	if (it.live) {
		const double* src = stage + it.stage;
		const int n = it.width * M;
		double v[M];
#pragma unroll
		for (int k = 0; k < M; k++) v[k] = nt_load(src + (unsigned)min(lane + kTileNodes * k, n - 1));
#pragma unroll
		for (int k = 0; k < M; k++) tl[tile_slot<M>(lane + kTileNodes * k)] = v[k];
	}
	__syncthreads();
	if (it.live) {
		double* dst = cur + it.plane;
		double o[M];
#pragma unroll
		for (int c = 0; c < M; c++) o[c] = tl[tile_slot<M>(lane * M + c)];
		if (lane < it.width) {
#pragma unroll
			for (int c = 0; c < M; c++) __builtin_nontemporal_store(o[c], dst + c * bx.cs + (unsigned)lane);
		}
	}
}

template <int M>
void pack(const double* cur, const StateBox& bx, int row0, unsigned items, double* stage_d, hipStream_t st) {
	hipLaunchKernelGGL(k_state_pack<M>, dim3((items + 3) / 4), dim3(256), 0, st, cur, bx, row0, items, stage_d);
}
template <int M>
void unpack(double* cur, const StateBox& bx, int row0, unsigned items, const double* stage_d, hipStream_t st) {
	hipLaunchKernelGGL(k_state_unpack<M>, dim3((items + 3) / 4), dim3(256), 0, st, cur, bx, row0, items, stage_d);
}

}  // namespace

StateBox make_state_box(const Geo& g, const int mn[3], const int mx[3]) {
	const int D = g.D, F = D - 1;
	StateBox bx{};
	bx.cs = g.cs;
	bx.na = bx.nb = 1;
	bx.base = g.origin + mn[F];
	bx.nf = mx[F] - mn[F];
	if (D >= 2) {
		bx.na = mx[0] - mn[0];
		bx.sa = g.stride[0];
		bx.base += (long long)mn[0] * g.stride[0];
	}
	if (D == 3) {
		bx.nb = mx[1] - mn[1];
		bx.sb = g.stride[1];
		bx.base += (long long)mn[1] * g.stride[1];
	}
	bx.tf = (bx.nf + kTileNodes - 1) / kTileNodes;
	return bx;
}

long long state_max_rows(const StateBox& bx) { return std::max<long long>(1, (1LL << 30) / bx.tf); }

bool launch_state_pack(const double* cur, int M, const StateBox& bx, long long row0, long long rows, double* stage_d,
                       hipStream_t st) {
	const unsigned items = (unsigned)(rows * bx.tf);
	switch (M) {
	case 2: pack<2>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 3: pack<3>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 4: pack<4>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 5: pack<5>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 9: pack<9>(cur, bx, (int)row0, items, stage_d, st); return true;
	}
	return false;
}

bool launch_state_unpack(double* cur, int M, const StateBox& bx, long long row0, long long rows,
                         const double* stage_d, hipStream_t st) {
	const unsigned items = (unsigned)(rows * bx.tf);
	switch (M) {
	case 2: unpack<2>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 3: unpack<3>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 4: unpack<4>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 5: unpack<5>(cur, bx, (int)row0, items, stage_d, st); return true;
	case 9: unpack<9>(cur, bx, (int)row0, items, stage_d, st); return true;
	}
	return false;
}

}  // namespace gcmx
