// state.hpp -- launchers of the state kernels (kernels_state.hip): the exact
// fp64 state of a box of a layer, moved between the layer's component planes
// (SoA) and a staging buffer in the reference's node order (AoS, [node][M]),
// so that a host never transposes a layer or holds one in the SoA form.
//   k_state_pack<M>    planes -> staging   (gcmx_read_box)
//   k_state_unpack<M>  staging -> planes   (gcmx_write_box)
// Pure moves: no arithmetic touches a value, every bit pattern arrives as it was.
#pragma once

#include "common.hpp"

namespace gcmx {

// A box by role: F the layer's fastest axis (z in 3-D, y in 2-D, x in 1-D), B
// the axis above it in 3-D (y), A the slowest (x) above 1-D.  A row of the box
// is its nf nodes of one (a, b): nf * M consecutive doubles of the AoS side.
// Rows are numbered a * nb + b, the AoS order.
struct StateBox {
	long long base;    // element offset of the box's first node in a component plane
	long long sa, sb;  // layer element strides of A and B
	long long cs;      // component stride
	int na, nb, nf;    // extents (1 for a role the dimension lacks)
	int tf;            // 64-node tiles of a row
};

// `mn`, `mx`: per axis of the context (entries >= D ignored); indices count from
// inner node 0 and may be negative (ghosts).
StateBox make_state_box(const Geo& g, const int mn[3], const int mx[3]);

// Most rows one launch takes (its tiles fit a 32-bit grid).
long long state_max_rows(const StateBox& bx);

// Rows [row0, row0 + rows) of the box: stage_d holds them as [rows * nf][M].
// False: no instance for this M (nothing was launched).
bool launch_state_pack(const double* cur, int M, const StateBox& bx, long long row0, long long rows, double* stage_d,
                       hipStream_t st);
bool launch_state_unpack(double* cur, int M, const StateBox& bx, long long row0, long long rows,
                         const double* stage_d, hipStream_t st);

}  // namespace gcmx
