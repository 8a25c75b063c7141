// kernels_ortho.hip -- the one-pass 3-D time step for unrotated orthotropic
// elastic media: X, Y and Z stages of cubic::Engine::nextTimeStep
// (Engine.cpp:90-121) in one kernel, in the block shape of k_fused_xyz
// (kernels_xyz.hip).  Arithmetic identical to k_stage_generic / the reference
// stage (engine/cubic/GridCharacteristicMethod.hpp:42-52) through onode_update
// (ortho.hpp).
#include "ortho.hpp"

#include <string>
#include <type_traits>

namespace gcmx {
// Compiled twice (Makefile), as kernels_xyz.hip is: the exact build
// (ortho_exact, -ffp-contract=off: the reference's separate multiply and add
// roundings, bitwise equal to the oracle) and the FMA build (ortho_fma,
// -DGCMX_FMA=1 -ffp-contract=fast; Lagrange form of the interpolant when
// floor(q) = 0 and bs <= 2).  gcmx_set_fp_mode selects one.
#ifndef GCMX_FMA
#define GCMX_FMA 0
#endif
#if GCMX_FMA
#define GCMX_ORTHO_NS ortho_fma
#define GCMX_FP_TAG ", FMA"
#else
#define GCMX_ORTHO_NS ortho_exact
#define GCMX_FP_TAG ""
#endif
namespace GCMX_ORTHO_NS {

// Block = one x plane, a chunk of y rows and the whole z row.  Each thread
// marches y; at row y it
//   * computes the X stage of row y+BS straight from the input layer (its
//     2*BS+1 x-neighbours are plain loads, one characteristic pair in flight at
//     a time; the neighbouring planes' blocks read the same lines from L2),
//   * pushes that X result into a register window of 2*BS+1 rows of the six
//     window components (the three node-only components of rows y..y+BS wait in
//     a delay line) and runs the Y stage of row y,
//   * hands the Y result to the Z stage through double-buffered LDS rows with
//     zeroed ghost slots, one barrier per row.
// HBM traffic: the input layer once, the output layer once (144 B/node/step).
// The loop is rotated as k_fused_xyz's: the first pair of the next X row is
// issued before this row's non-temporal stores, so its wait never includes them.
// Each axis has its own table with three distinct speeds (no UNI instance); the
// three OrthoAxis are kernel arguments the compiler re-fetches per stage.
// Instances: BS 1..3 x ZT 64..1024 (2*BS <= Z <= 1024), except BS = 3 with
// ZT = 1024 (ortho_supported); KF0: every pair of every axis has floor(q) = 0.
// Precondition: every y/z ghost of both layers is zero, so the intermediate
// results at ghost rows / columns are the constant 0.0; x ghost planes of `in`
// are valid.  Lanes z >= Z shadow column Z-1 and store 0.0 into the first z ghost.
//
// HET: per-node materials (GridCharacteristicMethod::stage takes each node's own
// matrices; the neighbours only supply values).  The materials' tables
// (het.n x 3 OrthoAxis, 720 B each) are copied into LDS at block start, one
// barrier before first use, so the row loop reads no table through global
// memory or the kernel arguments.  The id of row r (one byte
// per inner node, linear [x][y][z], no ghosts) is loaded with that row's first
// X-stage pair and travels to the row's Y and Z stages in a register ring
// beside `cen`; 145 B/node/step.  Rows >= Y (zero ghost rows, clamp_row) take
// the id of row Y-1 and lanes z >= Z that of column Z-1: any valid material maps
// a zero row to zero, a stray byte would index LDS past the tables.  AX/AY/AZ
// are unused; KF0 only (every pair of every axis of every material).  The
// per-lane coefficients live in VGPRs, so these instances are compiled for two
// waves per SIMD up to ZT = 512 (ortho_min_waves); instances: ortho_het_built.
//
// The LDS tables of one instance: declared only in the HET instantiation (the
// homogeneous instances keep their LDS size), one array per kernel instance.
template <int BS, int ZT, bool HET>
__device__ __forceinline__ OrthoAxis (*ortho_lds_tables())[3] {
	if constexpr (HET) {
		__shared__ OrthoAxis t[kHetMaxMaterials][3];
		return t;
	} else {
		return nullptr;
	}
}

template <int BS, int ZT, bool KF0, bool HET = false>
__global__ __launch_bounds__(ZT, ortho_min_waves(BS, ZT, HET)) void k_step_ortho(
    const double* __restrict__ in, double* __restrict__ outl, Geo g, OrthoAxis AX, OrthoAxis AY, OrthoAxis AZ, int x0,
    int chunk, int nplanes, OrthoHet het) {
	static_assert(!HET || KF0, "the heterogeneous step is built for floor(q) = 0 only");
	constexpr unsigned WMX = ortho_window(0);
	constexpr unsigned CMX = ortho_center_only(0);
	constexpr unsigned WMY = ortho_window(1);
	constexpr unsigned CMY = ortho_center_only(1);
	constexpr int NWY = popc9(WMY);
	constexpr int NCY = popc9(CMY);
	constexpr unsigned WMZ = ortho_window(2);
	constexpr int NWZ = popc9(WMZ);
	constexpr int W = 2 * BS + 1;
	constexpr int LW = ZT + 2 * BS;
	__shared__ double lds[2][NWZ][LW];

	const int z = threadIdx.x;
	const int Y = g.sizes[1], Z = g.sizes[2];
	// 1-D grid of nchunks * nplanes blocks in XCD-contiguous chunk-major order
	// (xcd_order): the x-neighbour planes a block re-reads were loaded by blocks
	// of the same XCD.  Placement only; any mapping is correct.
	int x, yb;
	{
		const int nx = (int)nplanes, T = (int)gridDim.x, b = (int)blockIdx.x;
		const int p = xcd_order(b, T);
		x = x0 + p % nx;
		yb = (p / nx) * chunk;
	}
	const int ye = min(yb + chunk, Y);
	const bool live = z < Z;
	const int zc = live ? z : Z - 1;  // idle lanes shadow a valid column
	const unsigned stx = (unsigned)g.stride[0];
	const unsigned sty = (unsigned)g.stride[1];
	// Plane bases in SGPRs at this block's plane x, 32-bit element offsets
	// relative to them (onepass_layout_ok)
	const long long pbase = (long long)x * g.stride[0];
	const unsigned plane = (unsigned)g.origin;  // node (x, 0, 0) from the bases
	const unsigned base = plane + zc;
	const Planes src(in + pbase, g.cs);
	const PlanesW out_p(outl + pbase, g.cs);

	// HET: the tables into LDS; ax(S, m): axis S of material m
	OrthoAxis(*const tabs)[3] = ortho_lds_tables<BS, ZT, HET>();
	[[maybe_unused]] const uint8_t* idp = nullptr;
	if constexpr (HET) {
		typedef unsigned long long u64;
		static_assert(sizeof(OrthoAxis) % sizeof(u64) == 0, "OrthoAxis is copied in 8-byte words");
		const int nw = het.n * 3 * (int)(sizeof(OrthoAxis) / sizeof(u64));
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
	auto ax = [&](auto SC, [[maybe_unused]] int m) -> const OrthoAxis& {
		constexpr int S = decltype(SC)::value;
		if constexpr (HET) return tabs[m][S];
		else return S == 0 ? AX : S == 1 ? AY : AZ;
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
	// windows) at a time with the next pair in flight.
	typedef double PairWin[2][W];
	auto pair_load = [&](auto PC, PairWin& w, unsigned o) {
		constexpr int P = decltype(PC)::value;
#pragma unroll
		for (int k = 0; k < W; k++) {
			w[0][k] = src.ld(opair_vel(0, P), o + (unsigned)(k - BS) * stx);
			w[1][k] = src.ld(opair_sig(0, P), o + (unsigned)(k - BS) * stx);
		}
	};
	auto pair_acc = [&](auto PC, const PairWin& w) {
		constexpr int P = decltype(PC)::value;
		return [&w](int j, int o) { return j == opair_vel(0, P) ? w[0][BS + o] : w[1][BS + o]; };
	};
	auto sched_fence = [] { __builtin_amdgcn_sched_barrier(0); };
	using P0 = std::integral_constant<int, 0>;
	using P1 = std::integral_constant<int, 1>;
	using P2 = std::integral_constant<int, 2>;
	// wa holds pair 0 of row r (already issued); loads pairs 1, 2 and the
	// node-only components as it goes.
	auto x_stage_rest = [&](PairWin& wa, int r, double (&xr)[9], int m) {
		const OrthoAxis& AX = ax(S0{}, m);
		const unsigned o = base + (unsigned)r * sty;
		PairWin wb;
		pair_load(P1{}, wb, o);
		double rr[9], n0[9], cv[9];
		opair_update<0, BS, KF0, 0>(AX, pair_acc(P0{}, wa), rr[0], rr[1]);
		n0[opair_vel(0, 0)] = wa[0][BS];
		n0[opair_sig(0, 0)] = wa[1][BS];
		sched_fence();
		pair_load(P2{}, wa, o);
		opair_update<0, BS, KF0, 1>(AX, pair_acc(P1{}, wb), rr[2], rr[3]);
		n0[opair_vel(0, 1)] = wb[0][BS];
		n0[opair_sig(0, 1)] = wb[1][BS];
		sched_fence();
#pragma unroll
		for (int j = 0; j < 9; j++)
			if ((CMX >> j) & 1u) cv[j] = src.ld(j, o);
		opair_update<0, BS, KF0, 2>(AX, pair_acc(P2{}, wa), rr[4], rr[5]);
		n0[opair_vel(0, 2)] = wa[0][BS];
		n0[opair_sig(0, 2)] = wa[1][BS];
		sched_fence();
		ocenter_update<0>(AX, [&](int j) { return ((WMX >> j) & 1u) ? n0[j] : cv[j]; }, rr);
		ou1_apply<0>(AX, rr, xr);
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
	// prologue: X results of rows yb-BS .. yb+BS (rows outside [0, Y) are zero
	// ghost rows)
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
	// in-loop X rows are loaded without a branch: rows past Y are zero ghost rows
	// (their X stage is 0.0), clamped into the plane's allocated ghost rows
	auto clamp_row = [&](int r) { return r < Y + BS - 1 ? r : Y + BS - 1; };
	const unsigned zo = live ? (unsigned)z : (unsigned)Z;

	int buf = 0;
	for (int y = yb; y < ye; y++) {
		double yv[9];
		int m_y = 0;
		if constexpr (HET) m_y = idr[0];
		const OrthoAxis& AYn = ax(S1{}, m_y);
		const OrthoAxis& AZn = ax(S2{}, m_y);
		onode_update<1, BS, KF0>(
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
			onode_update<2, BS, KF0>(
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

// ------------------------------------------------------------- launchers --

// The instance a launch runs, as a readable symbol (gcmx_profile_kernel).
template <int BS, int ZT, bool KF0, bool HET = false>
static const char* ortho_name() {
	static const std::string s = "k_step_ortho<" + std::to_string(BS) + ", " + std::to_string(ZT) + ", " +
	                             (KF0 ? "KF0" : "!KF0") + (HET ? ", HET" : "") + GCMX_FP_TAG + ">";
	return s.c_str();
}

// Rows per block, k_fused_xyz's rule (kernels_xyz.hip: xyz_chunk_for) restated:
// 128 while the launch still has >= 1024 blocks; thinner launches (X slabs, the
// boundary planes) halve it, down to 16 rows, to keep every CU busy.  Each block
// recomputes 2*BS X rows in its prologue.  `req` > 0 forces a value.
static int ortho_chunk_for(int Y, int nplanes, int req) {
	int chunk = req > 0 ? req : 128;
	if (req <= 0)
		while (chunk > 16 && (long long)((Y + chunk - 1) / chunk) * nplanes < 1024) chunk /= 2;
	return Y <= chunk ? Y : chunk;
}

template <int BS, int ZT>
static void launch_ortho_t(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                           hipStream_t st, int req_chunk, const char** kname, const OrthoHet* het) {
	const int chunk = ortho_chunk_for(g.sizes[1], x1 - x0, req_chunk);
	const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * (x1 - x0));
	if (het) {  // per-node materials: the caller checked floor(q) = 0 for every material
		if constexpr (ortho_het_built(BS, ZT)) {
			const OrthoAxis none{};
			hipLaunchKernelGGL((k_step_ortho<BS, ZT, true, true>), grid, dim3(ZT), 0, st, in, out, g, none, none, none,
			                   x0, chunk, x1 - x0, *het);
			*kname = ortho_name<BS, ZT, true, true>();
		}
		return;
	}
	bool kf0 = true;
	for (int s = 0; s < 3; s++)
		for (int p = 0; p < 3; p++) kf0 = kf0 && a[s].kf[p] == 0;
	const OrthoHet nohet{};
	if (kf0) {
		hipLaunchKernelGGL((k_step_ortho<BS, ZT, true>), grid, dim3(ZT), 0, st, in, out, g, a[0], a[1], a[2], x0,
		                   chunk, x1 - x0, nohet);
		*kname = ortho_name<BS, ZT, true>();
	} else {
		hipLaunchKernelGGL((k_step_ortho<BS, ZT, false>), grid, dim3(ZT), 0, st, in, out, g, a[0], a[1], a[2], x0,
		                   chunk, x1 - x0, nohet);
		*kname = ortho_name<BS, ZT, false>();
	}
}

template <int BS>
static void launch_ortho_bs(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                            hipStream_t st, int ch, const char** kn, const OrthoHet* het) {
	const int Z = g.sizes[2];
	if (Z <= 64) launch_ortho_t<BS, 64>(in, out, g, a, x0, x1, st, ch, kn, het);
	else if (Z <= 128) launch_ortho_t<BS, 128>(in, out, g, a, x0, x1, st, ch, kn, het);
	else if (Z <= 256) launch_ortho_t<BS, 256>(in, out, g, a, x0, x1, st, ch, kn, het);
	else if (Z <= 512) launch_ortho_t<BS, 512>(in, out, g, a, x0, x1, st, ch, kn, het);
	else if constexpr (BS <= 2) launch_ortho_t<BS, 1024>(in, out, g, a, x0, x1, st, ch, kn, het);
}

bool launch_step_ortho(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                       hipStream_t st, int chunk, const char** kname, int xb0, int xb1, const OrthoHet* het) {
	const char* dummy = nullptr;
	const char** kn = kname ? kname : &dummy;
	if (!ortho_supported(g) || x0 < 0 || x1 <= x0 || x1 > g.sizes[0] || chunk < 0) return false;
	if (het && (!ortho_het_supported(g) || !het->tab || !het->ids || het->n < 1 || het->n > kHetMaxMaterials))
		return false;
	if (!het && !a) return false;
	if (xb1 > xb0 && (xb0 < x1 || xb1 > g.sizes[0])) return false;  // range B after range A
	for (int r = 0; r < 2; r++) {
		if (r == 1) {  // no second range in the kernel: a second launch
			if (xb1 <= xb0) break;
			x0 = xb0;
			x1 = xb1;
		}
		switch (g.bs) {
		case 1: launch_ortho_bs<1>(in, out, g, a, x0, x1, st, chunk, kn, het); break;
		case 2: launch_ortho_bs<2>(in, out, g, a, x0, x1, st, chunk, kn, het); break;
		case 3: launch_ortho_bs<3>(in, out, g, a, x0, x1, st, chunk, kn, het); break;
		default: return false;
		}
	}
	return true;
}

}  // namespace GCMX_ORTHO_NS

#if !GCMX_FMA
// A 1024-thread block runs at 4 waves per SIMD, i.e. within 128 VGPRs, and the
// borderSize-3 windows do not fit them (the instance spilled 79 VGPRs to
// scratch): borderSize 3 takes rows up to 512 nodes, longer ones the generic stages.
bool ortho_supported(const Geo& g) { return fused_supported(g) && !(g.bs >= 3 && g.sizes[2] > 512); }
// The per-node-material instances (ortho_het_built).
bool ortho_het_supported(const Geo& g) {
	if (!ortho_supported(g) || g.bs < 1 || g.bs > 3) return false;
	const int Z = g.sizes[2];
	return ortho_het_built(g.bs, Z <= 64 ? 64 : Z <= 128 ? 128 : Z <= 256 ? 256 : Z <= 512 ? 512 : 1024);
}
#endif
}  // namespace gcmx
