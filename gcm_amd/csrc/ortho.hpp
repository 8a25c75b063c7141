// ortho.hpp -- structure of the unrotated orthotropic-elastic stage
// (ElasticModel<3>::constructNotRotated, ElasticModel3D.cpp:286-429) for the
// one-pass orthotropic step (kernels_ortho.hip), beside iso.hpp's isotropic one.
//
// Per axis S the decomposition has three characteristic pairs (rows 2p, 2p+1 of
// U, p = 0, 1: shear, p = 2: longitudinal), each reading one velocity and one
// stress component at the feet, with L = (-, +) within a pair, and three zero
// modes that read node values only:
//
//   axis | pair 0         | pair 1         | pair 2         | rows 6, 7, 8 read
//   x    | (Vy, Sxy, c66) | (Vz, Sxz, c55) | (Vx, Sxx, c11) | g0 Sxx + Syy; Syz; g1 Sxx + Szz
//   y    | (Vx, Sxy, c66) | (Vz, Syz, c44) | (Vy, Syy, c22) | Sxx + g0 Syy; Sxz; g1 Syy + Szz
//   z    | (Vx, Sxz, c55) | (Vy, Syz, c44) | (Vz, Szz, c33) | Sxx + g0 Szz; Sxy; Syy + g1 Szz
//
// The components read at the feet are the isotropic stage's (iso_window); the
// row order, the coefficients and the three distinct speeds per axis are not.
#pragma once

#include "iso.hpp"

namespace gcmx {

// Per-axis values of the orthotropic step, passed by value (kernel arguments).
struct OrthoAxis {
	double a[3];     // U:  stress entry of row 2p (row 2p+1 carries -a[p])
	double g[2];     // U:  the longitudinal-stress entries of rows 6 and 8
	double p[3];     // U1: stress-row entry of column 2p (column 2p+1 carries -p[p])
	double e[2];     // U1: column 4 entries of the rows of rows 6 / 8's unit components (column 5: -e)
	double c[3][3];  // per pair: ((q - i) + 1) / i, i = 1..bs
	double w[3][3];  // per pair: the interpolant's Lagrange weights (lagrange_weights)
	int kf[3];       // per pair: floor(q)
	int pad_;
};
static_assert(sizeof(OrthoAxis) == 28 * 8 + 4 * 4, "OrthoAxis has padding");

// Succeeds only for the exact pattern above (see the definition, gcmx.hip).
bool ortho_axis_extract(int s, const double* U, const double* U1, const double* L, OrthoAxis& A);

// The one-pass orthotropic step of planes [x0, x1) and, when xb1 > xb0, of a
// second range [xb0, xb1) (a second launch).  `a`: the three axes; `chunk`: y
// rows per block (0 = automatic).  Needs ortho_supported(g), y/z ghosts of both
// layers zero, x ghost planes of `in` valid.  Two builds, as kernels_xyz.hip's.
bool ortho_supported(const Geo& g);  // fused_supported(g), and Z <= 512 at borderSize 3
// Per-node materials for the step (the HET instances): per material three
// OrthoAxis (x, y, z; every pair with floor(q) = 0, its feet on the sides the
// kernel reads), at most kHetMaxMaterials of them, and the device ids of the
// inner nodes in linear [x][y][z] order (gcmx_set_material_ids' layout).  Then
// `a` is unused and may be null.
using OrthoHet = PlaneHet<OrthoAxis>;  // tab: [n][3], device
// The HET instances: borderSize 1..3 with rows up to 512 nodes, borderSize 1
// also up to 1024.  A 1024-thread block leaves 128 VGPRs, within which the
// per-lane coefficients do not fit beside the borderSize-2 windows (the instance
// spilled 4 VGPRs, 20 B/lane of scratch; the FMA build 12, 28 B/lane; DESIGN.md
// §3.10): borderSize >= 2 with rows longer than 512 keeps the generic stages.
__host__ __device__ constexpr bool ortho_het_built(int bs, int zt) {
	return bs >= 1 && bs <= 3 && zt <= 1024 && !(bs >= 2 && zt > 512);
}
bool ortho_het_supported(const Geo& g);  // ortho_supported(g) and the instance is built
// Minimum waves per SIMD of an instance: 4 (128 VGPRs) at borderSize <= 2, 2 at 3;
// the HET instances hold per-lane coefficients in VGPRs and take 2 where the
// block size allows it (one 512-thread block per CU).
__host__ __device__ constexpr int ortho_min_waves(int bs, int zt, bool het) {
	return het ? (zt > 512 ? 4 : 2) : (bs >= 3 ? 2 : 4);
}
namespace ortho_exact {
bool launch_step_ortho(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                       hipStream_t st, int chunk = 0, const char** kname = nullptr, int xb0 = 0, int xb1 = 0,
                       const OrthoHet* het = nullptr);
}
namespace ortho_fma {
bool launch_step_ortho(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                       hipStream_t st, int chunk = 0, const char** kname = nullptr, int xb0 = 0, int xb1 = 0,
                       const OrthoHet* het = nullptr);
}

// ----------------------------------------------------------- structure --

// Slots of the material values (beside iso.hpp's kZero / kOne / kHalf).
enum OrthoSlot : int { kOA = 16, kOG = 20, kOP = 24, kOE = 28 };  // + index

// Velocity / stress component of pair P; the stress components no pair reads,
// ascending (rows 6, 7, 8 carry a unit entry there).
__host__ __device__ constexpr int opair_vel(int S, int P) {
	return S == 0 ? (P == 0 ? 1 : P == 1 ? 2 : 0) : S == 1 ? (P == 0 ? 0 : P == 1 ? 2 : 1) : P;
}
__host__ __device__ constexpr int opair_sig(int S, int P) {
	return sig3(S, opair_vel(S, P));
}
__host__ __device__ constexpr int ozero_comp(int S, int i) {
	return S == 0 ? (i == 0 ? 6 : i == 1 ? 7 : 8) : S == 1 ? (i == 0 ? 3 : i == 1 ? 5 : 8) : (i == 0 ? 3 : i == 1 ? 4 : 6);
}

// U(k, j): rows are eigenstrings.
__host__ __device__ constexpr Coef ortho_u(int S, int k, int j) {
	if (k < 6) {
		const int p = k / 2;
		return j == opair_vel(S, p) ? Coef{kOne, 1} : j == opair_sig(S, p) ? Coef{kOA + p, (k & 1) ? -1 : 1} : cz();
	}
	if (j == ozero_comp(S, k - 6)) return Coef{kOne, 1};
	if (k != 7 && j == opair_sig(S, 2)) return Coef{kOG + (k == 8), 1};
	return cz();
}

// U1(c, n): columns are eigenvectors.
__host__ __device__ constexpr Coef ortho_u1(int S, int c, int n) {
	for (int p = 0; p < 3; p++) {
		if (c == opair_vel(S, p)) return (n == 2 * p || n == 2 * p + 1) ? Coef{kHalf, 1} : cz();
		if (c == opair_sig(S, p)) return n == 2 * p ? Coef{kOP + p, 1} : n == 2 * p + 1 ? Coef{kOP + p, -1} : cz();
	}
	for (int i = 0; i < 3; i++)
		if (c == ozero_comp(S, i)) {
			if (n == 6 + i) return Coef{kOne, 1};
			if (i != 1 && n == 4) return Coef{kOE + (i == 2), 1};
			if (i != 1 && n == 5) return Coef{kOE + (i == 2), -1};
		}
	return cz();
}

// The orthotropic stage for iso.hpp's stage templates: row 2P has L < 0, its
// foot on the +S side; every pair has its own speed.
template <>
struct Stage<OrthoAxis> {
	static constexpr int M = 9, NP = 3, kFoot = 1;
	__host__ __device__ static constexpr Coef u(int S, int k, int j) { return ortho_u(S, k, j); }
	__host__ __device__ static constexpr Coef u1(int S, int c, int n) { return ortho_u1(S, c, n); }
	// Components read at the neighbours (rows 0..5) / only at the node (rows 6..8).
	__host__ __device__ static constexpr unsigned window(int S) {
		unsigned m = 0;
		for (int p = 0; p < 3; p++) m |= bit(opair_vel(S, p)) | bit(opair_sig(S, p));
		return m;
	}
	__host__ __device__ static constexpr unsigned center_only(int S) {
		return bit(ozero_comp(S, 0)) | bit(ozero_comp(S, 1)) | bit(ozero_comp(S, 2));
	}
	__host__ __device__ static constexpr int pair_vel(int S, int P) { return opair_vel(S, P); }
	__host__ __device__ static constexpr int pair_sig(int S, int P) { return opair_sig(S, P); }
	// u * v for a structural entry; exact w.r.t. the reference product fl(u * v).
	template <int SLOT, int SIGN>
	__device__ __forceinline__ static double term(const OrthoAxis& A, double v) {
		double m;
		if constexpr (SLOT == kOne) m = v;
		else if constexpr (SLOT == kHalf) m = v * 0.5;
		else if constexpr (SLOT >= kOE) m = A.e[SLOT - kOE] * v;
		else if constexpr (SLOT >= kOP) m = A.p[SLOT - kOP] * v;
		else if constexpr (SLOT >= kOG) m = A.g[SLOT - kOG] * v;
		else m = A.a[SLOT - kOA] * v;
		return SIGN > 0 ? m : -m;
	}
	template <int P>
	__device__ __forceinline__ static const double* coef(const OrthoAxis& A) { return A.c[P]; }
	template <int P>
	__device__ __forceinline__ static const double* wts(const OrthoAxis& A) { return A.w[P]; }
	template <int P>
	__device__ __forceinline__ static int kf(const OrthoAxis& A) { return A.kf[P]; }
	// The one-plane step (plane_step.hpp): per-node materials are built; waves per SIMD.
	static constexpr bool kPlaneHet = true;
	__host__ __device__ static constexpr int plane_min_waves(int bs, int zt, bool het) {
		return ortho_min_waves(bs, zt, het);
	}
};
static_assert(Stage<OrthoAxis>::window(0) == iso_window(0) && Stage<OrthoAxis>::window(1) == iso_window(1) &&
                  Stage<OrthoAxis>::window(2) == iso_window(2),
              "the orthotropic stages read the isotropic window components");

}  // namespace gcmx
