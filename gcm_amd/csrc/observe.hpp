// observe.hpp -- launchers of the observation kernels (kernels_observe.hip):
// what a snapshotter or a detector needs from the current layer, formed on the
// device so that no call moves a whole layer to the host.
//   k_gather_q  quantities at listed nodes                 (gcmx_gather)
//   k_pack_vtk  the Float32 arrays of a box, VTK order     (gcmx_snapshot_box;
//               every k-th node per axis: gcmx_snapshot_strided)
//   k_scan      non-finite count and max |v| per component (gcmx_scan)
//   k_record    quantities at receivers into a device buffer (gcmx_record)
// Quantities are getQuantityOf's (host/task.hpp:134-143, host/acoustic_model.hpp:
// 145-180), bitwise: a component itself, or the elastic PRESSURE
//   trace = 0.0; trace += s_00; trace += s_11; ...; -trace / (double)D.
#pragma once

#include <cmath>

namespace gcmx {

// A point receiver (gcmx_recorder_create_points): the 2^dim nodes around a
// position in inner-index units and their multilinear weights.  Per axis d < dim
// (sizes[d] >= 2, 0 <= pos[d] <= sizes[d] - 1, else refused: NaN fails the range
// test) the base node is base[d] = min((int)floor(pos[d]), sizes[d] - 2) and
// t_d = pos[d] - (double)base[d], so the upper edge is base sizes - 2 with t = 1.
// Corner k in [0, 2^dim) lies at base[d] + receiver_corner_bit(dim, k, d) (the
// last axis runs fastest) with weight f_0, then * f_1, then * f_2, f_d = bit ?
// t_d : (1.0 - t_d), every product rounded on its own.  Host only and free of
// HIP: a stand-alone program built by a host compiler includes this file and
// sees this function alone (the launchers below need hipcc).
inline int receiver_corner_bit(int dim, int k, int d) { return (k >> (dim - 1 - d)) & 1; }
inline bool receiver_corners(int dim, const int* sizes, const double* pos, int base[3], double weight[8]) {
	if (dim < 1 || dim > 3) return false;
	double t[3] = {0.0, 0.0, 0.0};
	for (int d = 0; d < dim; d++) {
		if (sizes[d] < 2) return false;
		if (!(pos[d] >= 0.0 && pos[d] <= (double)(sizes[d] - 1))) return false;
		const int fl = (int)std::floor(pos[d]);
		base[d] = fl < sizes[d] - 2 ? fl : sizes[d] - 2;
		t[d] = pos[d] - (double)base[d];
	}
	for (int d = dim; d < 3; d++) base[d] = 0;
	for (int k = 0; k < (1 << dim); k++) {
		double w = receiver_corner_bit(dim, k, 0) ? t[0] : (1.0 - t[0]);
		for (int d = 1; d < dim; d++) w = w * (receiver_corner_bit(dim, k, d) ? t[d] : (1.0 - t[d]));
		weight[k] = w;
	}
	return true;
}

}  // namespace gcmx

#ifdef __HIPCC__

#include "common.hpp"
#include "launch.hpp"

namespace gcmx {

// Quantities of one observation call, by value (kernel arguments).
struct ObserveQ {
	int n;                  // quantities, <= kMaxBorderQ
	int comp[kMaxBorderQ];  // the component a quantity names, or kObservePressure
	int D;                  // terms of the elastic pressure's trace
	int diag[3];            // components of s_00, s_11, s_22
};
constexpr int kObservePressure = -1;

// out[q][i] = quantity q at element offset off_d[i] (origin included) of `cur`.
void launch_gather_q(const double* cur, const Geo& g, long long n, const long long* off_d,
                     const ObserveQ& oq, double* out_d, hipStream_t st);

// out[q][i] = quantity q at receiver i of `cur`: the value at element offset
// off_d[i] itself when K == 1 (w_d unused: bitwise launch_gather_q's), else
//   acc = w_d[i][0] * v_0;  acc = acc + w_d[i][k] * v_k  for ascending k < K,
// v_k the quantity at off_d[i][k] (the elastic PRESSURE per corner, then blended).
void launch_record(const double* cur, const Geo& g, long long n, int K, const long long* off_d, const double* w_d,
                   const ObserveQ& oq, double* out_d, hipStream_t st);

// The inner box [bmin, bmax) of `cur` as Float32 in VTK point order (x fastest,
// then y, then z): vel_d[n][3] when non-null (components >= D are 0.0f), then
// q_d[oq.n][n].  2-D and 3-D transpose through an LDS tile (the layer's fastest
// axis is the VTK order's slowest); 1-D copies.
void launch_pack_vtk(const double* cur, const Geo& g, const int bmin[3], const int bmax[3],
                     float* vel_d, const ObserveQ& oq, float* q_d, hipStream_t st);

// The same arrays over the lattice of every step[d]-th inner node from bmin: n[d]
// output points along axis d, point i_d is node bmin[d] + i_d * step[d] (the
// caller keeps the last one inside the inner box).  The STRIDED instance of
// k_pack_vtk: selected rows only along A and B; along F, the layer's contiguous
// axis, lane-strided 8-byte loads.  1-D: k_pack_line with the
// stride.
void launch_pack_vtk_strided(const double* cur, const Geo& g, const int bmin[3], const int n[3], const int step[3],
                             float* vel_d, const ObserveQ& oq, float* q_d, hipStream_t st);
// The compulsory traffic of that launch: HBM delivers whole 128-byte lines, so
// per selected row and fp64 plane read (`planes` per output point: Velocity's D, a
// trace's D, else 1) min(lines of the row's span, output points of the row) lines,
// plus the Float32 bytes written.
double pack_strided_traffic(const Geo& g, const int n[3], const int step[3], double planes, double out_bytes);

// res_d[0] = number of non-finite component values over the inner nodes (64-bit),
// res_d[1 + c] = bits of max |v| over the finite values of component c (0.0 when
// none).  Zeroes res_d on the stream first.
constexpr int kScanWords = 1 + kMaxM;
void launch_scan(const double* cur, const Geo& g, unsigned long long* res_d, hipStream_t st);

}  // namespace gcmx

#endif  // __HIPCC__
