// kernels_ortho.hip -- the one-pass 3-D time step for unrotated orthotropic
// elastic media: the one-plane kernel (plane_step.hpp) on ortho.hpp's stage,
// and its launcher.
#include "ortho.hpp"

#include <string>

// Compiled twice (Makefile), as kernels_xyz.hip is: the exact build
// (ortho_exact, -ffp-contract=off: the reference's separate multiply and add
// roundings, bitwise equal to the oracle) and the FMA build (ortho_fma,
// -DGCMX_FMA=1 -ffp-contract=fast; Lagrange form of the interpolant when
// floor(q) = 0 and bs <= 2).  gcmx_set_fp_mode selects one.
#ifndef GCMX_FMA
#define GCMX_FMA 0
#endif
#if GCMX_FMA
#define GCMX_BUILD_NS ortho_fma
#define GCMX_FP_TAG ", FMA"
#else
#define GCMX_BUILD_NS ortho_exact
#define GCMX_FP_TAG ""
#endif
#include "plane_step.hpp"

namespace gcmx {
namespace GCMX_BUILD_NS {

// ------------------------------------------------------------- launchers --

// The instance a launch runs, as a readable symbol (gcmx_profile_kernel): the
// one-plane kernel on the orthotropic stage is reported as k_step_ortho.
template <int BS, int ZT, bool KF0, bool HET = false>
static const char* ortho_name() {
	static const std::string s = "k_step_ortho<" + std::to_string(BS) + ", " + std::to_string(ZT) + ", " +
	                             (KF0 ? "KF0" : "!KF0") + (HET ? ", HET" : "") + GCMX_FP_TAG + ">";
	return s.c_str();
}

// Each axis has its own table with three distinct speeds, so there is no UNI
// instance.  Instances: BS 1..3 x ZT 64..1024 (2*BS <= Z <= 1024), except BS = 3
// with ZT = 1024 (ortho_supported); per-node materials: ortho_het_built, whose
// per-lane coefficients live in VGPRs, so they are compiled for two waves per
// SIMD up to ZT = 512 (ortho_min_waves).
template <int BS, int ZT>
static void launch_ortho_t(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                           hipStream_t st, int req_chunk, const char** kname, const OrthoHet* het) {
	const int chunk = plane_chunk_for(g.sizes[1], x1 - x0, req_chunk);
	const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * (x1 - x0));
	auto go = [&](auto KC, auto HC, const OrthoAxis* t, const OrthoHet& h) {
		constexpr bool K = decltype(KC)::value, H = decltype(HC)::value;
		hipLaunchKernelGGL((k_step_plane<OrthoAxis, BS, ZT, K, false, H>), grid, dim3(ZT), 0, st, in, out, g, t[0], t[1],
		                   t[2], x0, chunk, x1 - x0, h);
		*kname = ortho_name<BS, ZT, K, H>();
	};
	if (het) {  // per-node materials: the caller checked floor(q) = 0 for every material
		const OrthoAxis none[3] = {};
		if constexpr (ortho_het_built(BS, ZT)) go(std::true_type{}, std::true_type{}, none, *het);
		return;
	}
	bool kf0 = true;
	for (int s = 0; s < 3; s++)
		for (int p = 0; p < 3; p++) kf0 = kf0 && a[s].kf[p] == 0;
	if (kf0) go(std::true_type{}, std::false_type{}, a, OrthoHet{});
	else go(std::false_type{}, std::false_type{}, a, OrthoHet{});
}

template <int BS>
static void launch_ortho_bs(const double* in, double* out, const Geo& g, const OrthoAxis* a, int x0, int x1,
                            hipStream_t st, int ch, const char** kn, const OrthoHet* het) {
	with_row_lanes(g.sizes[2], [&](auto ZC) {
		constexpr int ZT = decltype(ZC)::value;
		if constexpr (BS <= 2 || ZT <= 512) launch_ortho_t<BS, ZT>(in, out, g, a, x0, x1, st, ch, kn, het);
	});
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

}  // namespace GCMX_BUILD_NS

#if !GCMX_FMA
// A 1024-thread block runs at 4 waves per SIMD, i.e. within 128 VGPRs, and the
// borderSize-3 windows do not fit them (the instance spilled 79 VGPRs to
// scratch): borderSize 3 takes rows up to 512 nodes, longer ones the generic stages.
bool ortho_supported(const Geo& g) { return fused_supported(g) && !(g.bs >= 3 && g.sizes[2] > 512); }
// The per-node-material instances (ortho_het_built).
bool ortho_het_supported(const Geo& g) {
	if (!ortho_supported(g) || g.bs < 1 || g.bs > 3) return false;
	return ortho_het_built(g.bs, row_lanes(g.sizes[2]));
}
#endif
}  // namespace gcmx
