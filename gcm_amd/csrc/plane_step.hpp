// plane_step.hpp -- the one-plane one-pass 3-D time step (X, Y and Z stages of
// cubic::Engine::nextTimeStep, Engine.cpp:90-121, in one kernel) for any medium
// with a Stage (iso.hpp): kernels_xyz.hip instantiates it for the isotropic
// medium (reported as k_fused_xyz<...>), kernels_ortho.hip for the orthotropic
// one (k_step_ortho<...>).  Arithmetic identical to k_stage_generic / the
// reference stage (engine/cubic/GridCharacteristicMethod.hpp:42-52) through
// pair_update / node_update.
//
// Both including files are compiled twice, exact and -DGCMX_FMA=1, and the
// kernel's body differs between the two (pair_update), so the template lives in
// the including file's build namespace, which it names in GCMX_BUILD_NS before
// the #include (xyz_exact, xyz_fma, ortho_exact, ortho_fma): in namespace gcmx
// the two objects would define one symbol and the linker would keep one body for
// both gcmx_set_fp_mode settings.  (Without the macro the launchers, which live
// in those namespaces, do not find the kernel: no build.)
#pragma once

#include "iso.hpp"

#include <type_traits>

namespace gcmx {
namespace GCMX_BUILD_NS {

// The materials' tables of a HET instance in LDS: declared only in the HET
// instantiation (the other instances keep their LDS size), one array per instance.
template <class AX, int BS, int ZT, bool HET>
__device__ __forceinline__ AX (*plane_lds_tables())[3] {
	if constexpr (HET) {
		__shared__ AX t[kHetMaxMaterials][3];
		return t;
	} else {
		return nullptr;
	}
}

// Block = one x plane, a chunk of y rows and the whole z row.  Each thread
// marches y; at row y it
//   * computes the X stage of row y+BS straight from the input layer (its
//     2*BS+1 x-neighbours are plain loads; the neighbouring planes' blocks read
//     the same lines, so they come from L2 / Infinity Cache, not HBM),
//   * pushes that X result into a register window of 2*BS+1 rows of the window
//     components (the node-only components of rows y..y+BS wait in a delay line)
//     and runs the Y stage of row y,
//   * hands the Y result to the Z stage through double-buffered LDS rows with
//     zeroed ghost slots, one barrier per row.
// HBM traffic: the input layer once, the output layer once (144 B/node/step).
// Reads `in` (all components, x ghost planes valid), writes `outl`.
//
// Schedule (measured A/B on MI355X): the loop is rotated (Y, Z,
// stores, then the X stage of the row that enters the window); the X stage
// loads one characteristic pair (10 values) at a time with the next pair in
// flight, which keeps the borderSize <= 2 instances at 128 VGPRs (two 512-thread
// blocks per CU); the first pair of the next row is issued before this row's
// stores, so its vmcnt wait never includes the stores (loads and stores retire
// in order on gfx950); the output is written with non-temporal stores.
// Precondition: every y/z ghost of both layers is zero, so the intermediate
// results at ghost rows / columns are the constant 0.0.  Lanes z >= Z shadow
// column Z-1 and store 0.0 into the first z ghost.
//
// AX: the medium's axis struct; the three axes' tables are kernel arguments the
// compiler re-fetches per stage.  KF0: every pair of every axis has floor(q) = 0.
// UNI: the launch has Z == ZT (no idle lanes) and the three tables are identical
// (isotropic medium, equal h): one table in scalar registers for all three
// stages and no idle-lane selects.  __launch_bounds__: Stage<AX>::plane_min_waves.
//
// HET (Stage<AX>::kPlaneHet): per-node materials (GridCharacteristicMethod::stage
// takes each node's own matrices; the neighbours only supply values).  The
// materials' tables (het.n x 3 AX) are copied into LDS at block start, one
// barrier before first use, so the row loop reads no table through global
// memory or the kernel arguments.  The id of row r (one byte
// per inner node, linear [x][y][z], no ghosts) is loaded with that row's first
// X-stage pair and travels to the row's Y and Z stages in a register ring
// beside `cen`; 145 B/node/step.  Rows >= Y (zero ghost rows, clamp_row) take
// the id of row Y-1 and lanes z >= Z that of column Z-1: any valid material maps
// a zero row to zero, a stray byte would index LDS past the tables.  AX_/AY_/AZ_
// are unused; KF0 only (every pair of every axis of every material).
template <class AX, int BS, int ZT, bool KF0, bool UNI, bool HET>
__global__ __launch_bounds__(ZT, Stage<AX>::plane_min_waves(BS, ZT, HET)) void k_step_plane(
    const double* __restrict__ in, double* __restrict__ outl, Geo g, AX AX_, AX AY_, AX AZ_, int x0, int chunk,
    int nplanes, PlaneHet<AX> het) {
	using ST = Stage<AX>;
	static_assert(!HET || ST::kPlaneHet, "per-node materials: not built for this medium");
	static_assert(!HET || (KF0 && !UNI), "the heterogeneous step is built for floor(q) = 0 only");
	constexpr unsigned WMX = ST::window(0);
	constexpr unsigned CMX = ST::center_only(0);
	constexpr unsigned WMY = ST::window(1);
	constexpr unsigned CMY = ST::center_only(1);
	constexpr int NWY = popc9(WMY);
	constexpr int NCY = popc9(CMY);
	constexpr unsigned WMZ = ST::window(2);
	constexpr int NWZ = popc9(WMZ);
	constexpr int W = 2 * BS + 1;
	constexpr int LW = ZT + 2 * BS;
	static_assert(NCY >= 1, "a delay line of node-only components");
	__shared__ double lds[2][NWZ][LW];

	const int z = threadIdx.x;
	const int Y = g.sizes[1], Z = g.sizes[2];
	// 1-D grid of nchunks * nplanes blocks.  Blocks are dealt round-robin over
	// the 8 XCDs (b % 8 share one, MI355X_MICROARCH.md §Workgroup dispatch): give
	// each XCD a contiguous run of (chunk, plane) pairs in chunk-major order, so
	// the 2*BS+1 x-neighbour planes a block re-reads were loaded by blocks of the
	// same XCD, i.e. hit its L2.  Placement only; any mapping is correct.
	int x, yb;
	{
		const int nx = (int)nplanes, T = (int)gridDim.x, b = (int)blockIdx.x;
		const int p = xcd_order(b, T);
		x = x0 + p % nx;
		yb = (p / nx) * chunk;
	}
	const int ye = min(yb + chunk, Y);
	const bool live = UNI || z < Z;
	const int zc = live ? z : Z - 1;  // idle lanes shadow a valid column
	const unsigned stx = (unsigned)g.stride[0];
	const unsigned sty = (unsigned)g.stride[1];
	// Plane bases in SGPRs at this block's plane x, element offsets relative to
	// them: 32-bit offsets whatever the layer's size (onepass_layout_ok)
	const long long pbase = (long long)x * g.stride[0];
	const unsigned plane = (unsigned)g.origin;  // node (x, 0, 0) from the bases
	const unsigned base = plane + zc;
	const Planes src(in + pbase, g.cs);
	const PlanesW out_p(outl + pbase, g.cs);

	// HET: the tables into LDS; ax(S, m): axis S of material m
	AX(*const tabs)[3] = plane_lds_tables<AX, BS, ZT, HET>();
	[[maybe_unused]] const uint8_t* idp = nullptr;
	if constexpr (HET) {
		typedef unsigned long long u64;
		static_assert(sizeof(AX) % sizeof(u64) == 0, "the tables are copied in 8-byte words");
		const int nw = het.n * 3 * (int)(sizeof(AX) / sizeof(u64));
		const u64* ts = reinterpret_cast<const u64*>(het.tab);
		u64* td = reinterpret_cast<u64*>(&tabs[0][0]);
		for (int i = z; i < nw; i += ZT) td[i] = ts[i];
		idp = het.ids + ((long long)x * Y) * Z + zc;
	}
	// the id of inner node (x, r, zc), r clamped into the id array (no ghosts)
	auto id_load = [&](int r) -> int {
		if constexpr (HET) return idp[(unsigned)(r < Y - 1 ? r : Y - 1) * (unsigned)Z];
		else return 0;
	};
	auto ax = [&](auto SC, [[maybe_unused]] int m) -> const AX& {
		constexpr int S = decltype(SC)::value;
		if constexpr (HET) return tabs[m][S];
		else return (UNI || S == 0) ? AX_ : S == 1 ? AY_ : AZ_;
	};
	using S0 = std::integral_constant<int, 0>;
	using S1 = std::integral_constant<int, 1>;
	using S2 = std::integral_constant<int, 2>;

	if (z < 2 * BS) {  // ghost slots of both LDS row buffers: zero, never overwritten
		const int gslot = (z < BS) ? z : (Z + z);
#pragma unroll
		for (int q = 0; q < NWZ; q++) {
			lds[0][q][gslot] = 0.0;
			lds[1][q][gslot] = 0.0;
		}
	}
	if constexpr (HET) __syncthreads();  // the tables, before the prologue's X stages

	// X stage of row r, loaded one characteristic pair (velocity + stress
	// windows, 10 values) at a time with the next pair in flight: at most two
	// pairs are live in registers.
	typedef double PairWin[2][W];
	auto pair_load = [&](auto PC, PairWin& w, unsigned o) {
		constexpr int P = decltype(PC)::value;
#pragma unroll
		for (int k = 0; k < W; k++) {
			w[0][k] = src.ld(ST::pair_vel(0, P), o + (unsigned)(k - BS) * stx);
			w[1][k] = src.ld(ST::pair_sig(0, P), o + (unsigned)(k - BS) * stx);
		}
	};
	auto pair_acc = [&](auto PC, const PairWin& w) {
		constexpr int P = decltype(PC)::value;
		return [&w](int j, int o) { return j == ST::pair_vel(0, P) ? w[0][BS + o] : w[1][BS + o]; };
	};
	auto sched_fence = [] { __builtin_amdgcn_sched_barrier(0); };
	using P0 = std::integral_constant<int, 0>;
	using P1 = std::integral_constant<int, 1>;
	using P2 = std::integral_constant<int, 2>;
	// wa holds pair 0 of row r (already issued); loads pairs 1, 2 and the
	// node-only components as it goes.
	auto x_stage_rest = [&](PairWin& wa, int r, double (&xr)[9], int m) {
		const AX& AXn = ax(S0{}, m);
		const unsigned o = base + (unsigned)r * sty;
		PairWin wb;
		pair_load(P1{}, wb, o);
		double rr[9], n0[9], cv[9];
		pair_update<0, BS, KF0, 0>(AXn, pair_acc(P0{}, wa), rr[0], rr[1]);
		n0[ST::pair_vel(0, 0)] = wa[0][BS];
		n0[ST::pair_sig(0, 0)] = wa[1][BS];
		sched_fence();
		pair_load(P2{}, wa, o);
		pair_update<0, BS, KF0, 1>(AXn, pair_acc(P1{}, wb), rr[2], rr[3]);
		n0[ST::pair_vel(0, 1)] = wb[0][BS];
		n0[ST::pair_sig(0, 1)] = wb[1][BS];
		sched_fence();
#pragma unroll
		for (int j = 0; j < 9; j++)
			if ((CMX >> j) & 1u) cv[j] = src.ld(j, o);
		pair_update<0, BS, KF0, 2>(AXn, pair_acc(P2{}, wa), rr[4], rr[5]);
		n0[ST::pair_vel(0, 2)] = wa[0][BS];
		n0[ST::pair_sig(0, 2)] = wa[1][BS];
		sched_fence();
		center_update<0>(AXn, [&](int j) { return ((WMX >> j) & 1u) ? n0[j] : cv[j]; }, rr);
		u1_apply<0>(AXn, rr, xr);
	};
	auto x_load_a = [&](PairWin& wa, int r) { pair_load(P0{}, wa, base + (unsigned)r * sty); };

	// Y window over X results of rows y-BS..y+BS; node-only components of rows
	// y..y+BS wait in a small delay line.
	double win[NWY][W];
	double cen[BS + 1][NCY];
	[[maybe_unused]] int idr[BS + 1];  // HET: ids of rows y..y+BS
	auto push = [&](const double (&xr)[9], int slot, [[maybe_unused]] int m) {  // slot: window index of the row
		if constexpr (HET) {
			if (slot >= BS) idr[slot - BS] = m;
		}
#pragma unroll
		for (int j = 0; j < 9; j++) {
			if ((WMY >> j) & 1u) win[wslot(WMY, j)][slot] = xr[j];
			if ((CMY >> j) & 1u) {
				if (slot >= BS) cen[slot - BS][wslot(CMY, j)] = xr[j];
			}
		}
	};
	// Rotated schedule: the loads of an X row are issued at the END of an
	// iteration and consumed after the next iteration's stores, so in every path
	// into the loop they are older than 9 stores and the compiler's vmcnt waits
	// never include the stores' completion.  Stores, LDS writes and the Z stage
	// are unconditional (idle lanes z >= Z write 0.0 into the first z ghost, which
	// the precondition keeps zero), and the in-loop X rows are loaded without a
	// branch: rows outside [0, Y) are zero ghost rows, clamped into the plane.
	// prologue: X results of rows yb-BS .. yb+BS
#pragma unroll
	for (int k = 0; k < W; k++) {
		const int r = yb - BS + k;
		double xr[9];
		int m = 0;
		if (r >= 0 && r < Y) {
			PairWin wa;
			x_load_a(wa, r);
			m = id_load(r);
			x_stage_rest(wa, r, xr, m);
		} else {
#pragma unroll
			for (int j = 0; j < 9; j++) xr[j] = 0.0;
		}  // (a zero row's id is never used: the Y and Z stages run for rows < Y only)
		push(xr, k, m);
	}
	auto clamp_row = [&](int r) { return r < Y + BS - 1 ? r : Y + BS - 1; };
	const unsigned zo = live ? (unsigned)z : (unsigned)Z;

	int buf = 0;
#pragma unroll 1
	for (int y = yb; y < ye; y++) {
		double yv[9];
		int m_y = 0;
		if constexpr (HET) m_y = idr[0];
		const AX& AYn = ax(S1{}, m_y);
		const AX& AZn = ax(S2{}, m_y);
		node_update<1, BS, KF0>(
		    AYn, [&](int j, int o) { return win[wslot(WMY, j)][BS + o]; },
		    [&](int j) { return ((WMY >> j) & 1u) ? win[wslot(WMY, j)][BS] : cen[0][wslot(CMY, j)]; }, yv);
#pragma unroll
		for (int j = 0; j < 9; j++)
			if ((WMZ >> j) & 1u) lds[buf][wslot(WMZ, j)][BS + z] = live ? yv[j] : 0.0;
		PairWin wa_next;
		[[maybe_unused]] int m_next = 0;
		__syncthreads();
		{
			double zv[9];
			node_update<2, BS, KF0>(
			    AZn, [&](int j, int o) { return lds[buf][wslot(WMZ, j)][BS + z + o]; },
			    [&](int j) { return ((WMZ >> j) & 1u) ? lds[buf][wslot(WMZ, j)][BS + z] : yv[j]; }, zv);
			const unsigned offo = plane + (unsigned)y * sty + zo;
			// next row's first pair: loads older than this row's stores
			sched_fence();
			x_load_a(wa_next, clamp_row(y + BS + 1));
			if constexpr (HET) m_next = id_load(y + BS + 1);
			sched_fence();
#pragma unroll
			for (int c = 0; c < 9; c++) out_p.st_nt(c, offo, live ? zv[c] : 0.0);
		}
		buf ^= 1;
#pragma unroll
		for (int q = 0; q < NWY; q++)
#pragma unroll
			for (int o = 0; o < W - 1; o++) win[q][o] = win[q][o + 1];
#pragma unroll
		for (int k = 0; k < BS; k++)
#pragma unroll
			for (int q = 0; q < NCY; q++) cen[k][q] = cen[k + 1][q];
		if constexpr (HET) {
#pragma unroll
			for (int k = 0; k < BS; k++) idr[k] = idr[k + 1];
		}
		{  // X stage of row y+BS+1 (zero ghost rows give zero) -> window slot W-1
			double xr[9];
			sched_fence();
			x_stage_rest(wa_next, clamp_row(y + BS + 1), xr, m_next);
			push(xr, W - 1, m_next);
			sched_fence();
		}
	}
}

}  // namespace GCMX_BUILD_NS
}  // namespace gcmx
