// kernels_acoustic.hip -- the one-pass 3-D time step for acoustic media: X, Y
// and Z stages of cubic::Engine::nextTimeStep (Engine.cpp:90-121) in one
// kernel, in the block shape of the one-plane kernel (plane_step.hpp).  Arithmetic
// identical to k_stage_generic / the reference stage
// (engine/cubic/GridCharacteristicMethod.hpp:42-52) through ac_pair (below).
// One build, -ffp-contract=off: the reference's separate multiply and add
// roundings (gcmx_set_fp_mode changes nothing on an acoustic context).
#include "acoustic.hpp"
#include "iso.hpp"
#include "launch.hpp"

#include <string>

namespace gcmx {

// The stage of axis S at one node: the two characteristic rows and U1's two
// non-trivial rows (acoustic.hpp).  V(o), P(o): the axis velocity and the
// pressure at offset o along S (|o| <= BS).  Sums run in ascending index order
// from the first non-zero term, as k_stage_generic's: velocity (index S < D)
// before pressure (index D), column 0 before column 1; the unit entries of U1
// multiply exactly.
template <int BS, bool KF0, class VF, class PF>
__device__ __forceinline__ void ac_pair(const AcAxis& A, VF V, PF P, double& v_out, double& p_out) {
	double sv[BS + 1], sp[BS + 1];
#pragma unroll
	for (int i = 0; i <= BS; i++) {
		sv[i] = V(-i);
		sp[i] = P(-i);
	}
	const double r0 = 0.5 * newton_minmax<BS, KF0>(sv, A.kf, A.c) + A.u0 * newton_minmax<BS, KF0>(sp, A.kf, A.c);
#pragma unroll
	for (int i = 0; i <= BS; i++) {
		sv[i] = V(i);
		sp[i] = P(i);
	}
	const double r1 = 0.5 * newton_minmax<BS, KF0>(sv, A.kf, A.c) + A.u1 * newton_minmax<BS, KF0>(sp, A.kf, A.c);
	v_out = r0 + r1;
	p_out = A.p0 * r0 + A.p1 * r1;
}

// Minimum waves per SIMD of an instance (profiles/acoustic/resource_usage.txt):
// the borderSize-1 instances fit 64 VGPRs (8 waves); within 64 the borderSize-2
// instances spilled 13-14 VGPRs and the borderSize-3 ones 70-80, so those are
// compiled for 4 waves (128 VGPRs; a 1024-thread block needs no more).
__host__ __device__ constexpr int acoustic_min_waves(int bs) { return bs <= 1 ? 8 : 4; }

// Block = one x plane, a chunk of y rows and the whole z row.  Each thread
// marches y; at row y it
//   * runs the Y stage of row y on a register window of 2*BS+1 rows: the X
//     result of p and the input's Vy (the X stage returns Vy unchanged, so it is
//     loaded, not carried); the X result of Vx and the input's Vz of rows
//     y..y+BS wait in a delay line,
//   * hands p'' and Vz to the Z stage through double-buffered LDS rows with
//     zeroed ghost slots, one barrier per row,
//   * runs the X stage of row y+BS+1 from the 2*BS+1 planes' Vx and p (plain
//     loads; the neighbouring planes' blocks read the same lines from L2) and
//     pushes it into the window.
// HBM traffic: the input layer once, the output layer once (64 B/node/step).
// The loop is rotated by a whole row: the loads of row y+BS+2 are issued
// before row y's non-temporal stores and consumed one iteration later, so their
// wait never includes the stores and spans a row's arithmetic.
// Precondition: every y/z ghost of both layers is zero, so the intermediate
// results at ghost rows / columns are the constant 0.0; x ghost planes of `in`
// are valid.  Lanes z >= Z shadow column Z-1 and store 0.0 into the first z ghost.
// KF0: floor(q) = 0 on every axis.
template <int BS, int ZT, bool KF0>
__global__ __launch_bounds__(ZT, acoustic_min_waves(BS)) void k_step_acoustic(
    const double* __restrict__ in, double* __restrict__ outl, Geo g, AcAxis AX, AcAxis AY, AcAxis AZ, int x0, int chunk,
    int nplanes) {
	constexpr int W = 2 * BS + 1;
	constexpr int LW = ZT + 2 * BS;
	__shared__ double lds[2][2][LW];  // [buffer][p'', Vz][slot]

	const int z = threadIdx.x;
	const int Y = g.sizes[1], Z = g.sizes[2];
	// 1-D grid of nchunks * nplanes blocks in XCD-contiguous chunk-major order
	// (xcd_order).  Placement only; any mapping is correct.
	int x, yb;
	{
		const int p = xcd_order((int)blockIdx.x, (int)gridDim.x);
		x = x0 + p % nplanes;
		yb = (p / nplanes) * chunk;
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
	const PlanesN<4> src(in + pbase, g.cs);  // the four component planes
	const PlanesWN<4> out_p(outl + pbase, g.cs);

	if (z < 2 * BS) {  // ghost slots of both LDS row buffers: zero, never overwritten
		const int gslot = (z < BS) ? z : (Z + z);
#pragma unroll
		for (int q = 0; q < 2; q++) {
			lds[0][q][gslot] = 0.0;
			lds[1][q][gslot] = 0.0;
		}
	}

	// The input of one row's X stage: Vx and p over the 2*BS+1 planes, Vy and Vz
	// at the node.
	struct RowIn {
		double vx[W], p[W], vy, vz;
	};
	auto row_load = [&](RowIn& w, int r) {
		const unsigned o = base + (unsigned)r * sty;
#pragma unroll
		for (int k = 0; k < W; k++) {
			w.vx[k] = src.ld(0, o + (unsigned)(k - BS) * stx);
			w.p[k] = src.ld(3, o + (unsigned)(k - BS) * stx);
		}
		w.vy = src.ld(1, o);
		w.vz = src.ld(2, o);
	};
	// Y window over rows y-BS..y+BS: the X result of p and the input's Vy; the X
	// result of Vx and the input's Vz of rows y..y+BS in a delay line.
	double wp[W], wvy[W], dvx[BS + 1], dvz[BS + 1];
	// X stage of a loaded row into window slot `slot`; `zero`: a ghost row, whose
	// X result is the constant 0.0 (its Vy and Vz are the zero ghosts themselves)
	auto x_push = [&](const RowIn& w, int slot, bool zero) {
		double xv, xp;
		ac_pair<BS, KF0>(AX, [&](int o) { return w.vx[BS + o]; }, [&](int o) { return w.p[BS + o]; }, xv, xp);
		wp[slot] = zero ? 0.0 : xp;
		wvy[slot] = zero ? 0.0 : w.vy;
		if (slot >= BS) {
			dvx[slot - BS] = zero ? 0.0 : xv;
			dvz[slot - BS] = zero ? 0.0 : w.vz;
		}
	};
	// rows are loaded without a branch: rows outside [0, Y) are zero ghost rows,
	// clamped into the plane's allocated ghost rows
	auto clamp_row = [&](int r) { return r < -BS ? -BS : r < Y + BS - 1 ? r : Y + BS - 1; };
	auto ghost_row = [&](int r) { return r < 0 || r >= Y; };

	// prologue: X results of rows yb-BS .. yb+BS
#pragma unroll
	for (int k = 0; k < W; k++) {
		const int r = yb - BS + k;
		RowIn w;
		row_load(w, clamp_row(r));
		x_push(w, k, ghost_row(r));
	}
	RowIn nx;  // row y+BS+1, in flight
	row_load(nx, clamp_row(yb + BS + 1));
	const unsigned zo = live ? (unsigned)z : (unsigned)Z;
	auto sched_fence = [] { __builtin_amdgcn_sched_barrier(0); };

	int buf = 0;
	for (int y = yb; y < ye; y++) {
		double yv, yp;
		ac_pair<BS, KF0>(AY, [&](int o) { return wvy[BS + o]; }, [&](int o) { return wp[BS + o]; }, yv, yp);
		const double vxo = dvx[0], vzn = dvz[0];
		lds[buf][0][BS + z] = live ? yp : 0.0;
		lds[buf][1][BS + z] = live ? vzn : 0.0;
		__syncthreads();
		double zv, zp;
		ac_pair<BS, KF0>(AZ, [&](int o) { return lds[buf][1][BS + z + o]; }, [&](int o) { return lds[buf][0][BS + z + o]; },
		                 zv, zp);
		buf ^= 1;
		// X stage of row y+BS+1 from the loads of the previous iteration
		double xv, xp;
		ac_pair<BS, KF0>(AX, [&](int o) { return nx.vx[BS + o]; }, [&](int o) { return nx.p[BS + o]; }, xv, xp);
		const bool zr = y + BS + 1 >= Y;
		const double nvy = nx.vy, nvz = nx.vz;
		// row y+BS+2's loads: older than this row's stores
		sched_fence();
		row_load(nx, clamp_row(y + BS + 2));
		sched_fence();
		const unsigned offo = plane + (unsigned)y * sty + zo;
		out_p.st_nt(0, offo, live ? vxo : 0.0);
		out_p.st_nt(1, offo, live ? yv : 0.0);
		out_p.st_nt(2, offo, live ? zv : 0.0);
		out_p.st_nt(3, offo, live ? zp : 0.0);
#pragma unroll
		for (int o = 0; o < W - 1; o++) {
			wp[o] = wp[o + 1];
			wvy[o] = wvy[o + 1];
		}
#pragma unroll
		for (int k = 0; k < BS; k++) {
			dvx[k] = dvx[k + 1];
			dvz[k] = dvz[k + 1];
		}
		wp[W - 1] = zr ? 0.0 : xp;
		wvy[W - 1] = zr ? 0.0 : nvy;
		dvx[BS] = zr ? 0.0 : xv;
		dvz[BS] = zr ? 0.0 : nvz;
	}
}

// ------------------------------------------------------------- launchers --

// The instance a launch runs, as a readable symbol (gcmx_profile_kernel).
template <int BS, int ZT, bool KF0>
static const char* acoustic_name() {
	static const std::string s =
	    "k_step_acoustic<" + std::to_string(BS) + ", " + std::to_string(ZT) + ", " + (KF0 ? "KF0" : "!KF0") + ">";
	return s.c_str();
}

template <int BS, int ZT>
static void launch_acoustic_t(const double* in, double* out, const Geo& g, const AcAxis* a, int x0, int x1,
                              hipStream_t st, int req_chunk, const char** kname) {
	const int chunk = plane_chunk_for(g.sizes[1], x1 - x0, req_chunk);
	const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * (x1 - x0));
	if (a[0].kf == 0 && a[1].kf == 0 && a[2].kf == 0) {
		hipLaunchKernelGGL((k_step_acoustic<BS, ZT, true>), grid, dim3(ZT), 0, st, in, out, g, a[0], a[1], a[2], x0,
		                   chunk, x1 - x0);
		*kname = acoustic_name<BS, ZT, true>();
	} else {
		hipLaunchKernelGGL((k_step_acoustic<BS, ZT, false>), grid, dim3(ZT), 0, st, in, out, g, a[0], a[1], a[2], x0,
		                   chunk, x1 - x0);
		*kname = acoustic_name<BS, ZT, false>();
	}
}

template <int BS>
static void launch_acoustic_bs(const double* in, double* out, const Geo& g, const AcAxis* a, int x0, int x1,
                               hipStream_t st, int ch, const char** kn) {
	with_row_lanes(g.sizes[2], [&](auto ZC) {
		launch_acoustic_t<BS, decltype(ZC)::value>(in, out, g, a, x0, x1, st, ch, kn);
	});
}

bool acoustic_supported(const Geo& g) { return fused_supported(g) && g.M == 4; }

bool launch_step_acoustic(const double* in, double* out, const Geo& g, const AcAxis* a, int x0, int x1,
                          hipStream_t st, int chunk, const char** kname) {
	const char* dummy = nullptr;
	const char** kn = kname ? kname : &dummy;
	if (!acoustic_supported(g) || !a || x0 < 0 || x1 <= x0 || x1 > g.sizes[0] || chunk < 0) return false;
	for (int s = 0; s < 3; s++)
		if (a[s].kf < 0 || a[s].kf >= g.bs) return false;
	switch (g.bs) {
	case 1: launch_acoustic_bs<1>(in, out, g, a, x0, x1, st, chunk, kn); break;
	case 2: launch_acoustic_bs<2>(in, out, g, a, x0, x1, st, chunk, kn); break;
	case 3: launch_acoustic_bs<3>(in, out, g, a, x0, x1, st, chunk, kn); break;
	default: return false;
	}
	return true;
}

}  // namespace gcmx
