// setup.hpp -- launchers of the set-up kernels (kernels_setup.hip): a body's
// initial state and material ids formed on the device from a short list of
// areas, so that set-up moves no layer from the host.
//   k_setup_state  InitialCondition::apply over an inner box   (gcmx_setup_state)
//   k_setup_ids    MaterialsCondition::apply over an inner box (gcmx_setup_material_ids),
//                  or, writing nothing, the ids that occur     (gcmx_setup_census)
// Coordinates are CubicGrid::coords' (host/engine.hpp), bitwise:
//   (double)start[i] * h[i] + (double)it[i] * h[i], 0.0 for axes >= D,
// and Area::contains is restated operation for operation from host/task.hpp, so
// a node on an area's surface falls on the side the host puts it.
#pragma once

#include "../../include/gcmx.h"
#include "common.hpp"

namespace gcmx {

constexpr int kSetupMaxAreas = GCMX_MAX_SETUP_AREAS;
constexpr int kAreaWords = 11;  // a gcmx_area as 64-bit words
static_assert(sizeof(gcmx_area) == kAreaWords * 8, "gcmx_area is 88 bytes");
// The tables of one call as 64-bit words: n areas, then n vectors of M doubles
// (state) or n id bytes (ids); the device buffer holds the largest.
constexpr size_t kSetupTableBytes = (size_t)kSetupMaxAreas * (kAreaWords + kMaxM) * 8;
constexpr int kCensusWords = 8;  // 256 bits: bit v of word v / 32 = id v occurs

// The box of a set-up launch by role: F the layer's fastest axis (z in 3-D, y in
// 2-D, x in 1-D), B the axis above it in 3-D (y), A the slowest (x) above 1-D.
// Indices a, b, f count from the box's minimum; it is those the coordinates are
// formed from, with the box's own start.
struct SetupBox {
	int D;
	int a0, b0, f0;     // the box's minimum (inner indices of the context)
	int na, nb, nf;     // extents (1 for a role the dimension lacks)
	long long sa, sb;   // layer element strides of A and B
	long long ma, mb;   // the same in the id array (linear inner order, no ghosts)
	int ga, gb, gf;     // start: global index of the box's first node
	double ha, hb, hf;  // spatial steps
	int nseg;           // 64-node segments of a row
	long long items;    // rows x segments: one per wave and turn
};

// `mn`, `mx`, `start`: per axis of the context (entries >= D ignored).
SetupBox make_setup_box(const Geo& g, const int mn[3], const int mx[3], const int start[3], const double h[3]);

// tab_d: n areas then vectors[n][M].  Writes the M component planes of `cur` at
// the box's nodes; nothing else.
void launch_setup_state(double* cur, const Geo& g, const SetupBox& bx, int n, const unsigned long long* tab_d,
                        hipStream_t st);
// tab_d: n areas then id_of[n] bytes.  mat_d non-null: one byte per node of the
// box into the id array.  Null: nothing is written but used_d[kCensusWords]
// (zeroed on the stream first), the mask of the ids that occur in the box.
void launch_setup_ids(uint8_t* mat_d, const Geo& g, const SetupBox& bx, int n, const unsigned long long* tab_d,
                      unsigned* used_d, hipStream_t st);

}  // namespace gcmx
