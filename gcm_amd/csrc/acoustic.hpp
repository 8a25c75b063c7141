// acoustic.hpp -- structure of the acoustic stage (AcousticModel<D>::
// constructGcmMatrix for the identity basis, rheology/models/AcousticModel.hpp:214-317)
// for the one-pass acoustic step (kernels_acoustic.hip), beside iso.hpp's and
// ortho.hpp's elastic ones.
//
// The PDE vector is Vx..V(D-1), then the pressure at index D (M = D + 1).  Per
// axis S the decomposition has one characteristic pair and D - 1 zero modes:
//
//   row 0: 0.5 V_S + u0 p,  L = +c (foot on the -S side)
//   row 1: 0.5 V_S + u1 p,  L = -c (foot on the +S side),  u1 = -u0
//   rows 2..D: +-1 on one tangential velocity each, L = 0 (node values)
//
//   U1 column 0: 1 on V_S, p0 on p;  column 1: 1 on V_S, p1 = -p0 on p;
//   columns 2..D: the zero modes' own +-1.
//
// A zero mode's two signs cancel exactly in U1 (U u), so a stage returns the
// tangential velocities bit for bit and forms only V_S and p anew.
#pragma once

#include "common.hpp"

namespace gcmx {

// Border quantity code kDirectQ + c names component c itself.  gcmx.hip's
// border_q turns an acoustic context's PRESSURE (12) into kDirectQ + D
// (AcousticVariables::QUANTITIES: the pressure is a component, not the trace of
// a stress); the border kernels' quantity_component resolves it.
constexpr int kDirectQ = 64;

// Per-axis values of the acoustic step, passed by value (kernel arguments).
struct AcAxis {
	double u0, u1;  // U:  pressure entries of rows 0 / 1
	double p0, p1;  // U1: pressure-row entries of columns 0 / 1
	double c[3];    // ((q - i) + 1) / i, i = 1..bs (both feet share q)
	int kf;         // floor(q)
	int pad_;
};
static_assert(sizeof(AcAxis) == 7 * 8 + 2 * 4, "AcAxis has padding");

// Succeeds only for the exact pattern above, entry by entry (gcmx.hip);
// M = D + 1, U / U1 row-major [M][M].
bool acoustic_axis_extract(int D, int s, const double* U, const double* U1, const double* L, AcAxis& A);

// The one-pass acoustic step needs fused_supported(g) (2*bs <= Z <= 1024,
// bs <= 3, 32-bit offsets within a block's planes) and g.M == 4.
bool acoustic_supported(const Geo& g);
// X, Y and Z stages of planes [x0, x1) in one pass; `a`: the three axes;
// `chunk`: y rows per block (0 = automatic).  Needs every y/z ghost of both
// layers zero and the x ghost planes of `in` valid.  `kname`: set to the
// launched instance's symbol (a static string).
bool launch_step_acoustic(const double* in, double* out, const Geo& g, const AcAxis* a, int x0, int x1,
                          hipStream_t st, int chunk = 0, const char** kname = nullptr);

}  // namespace gcmx
