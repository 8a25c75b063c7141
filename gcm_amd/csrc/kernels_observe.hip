// kernels_observe.hip -- observation of the current layer without moving it to
// the host (observe.hpp): quantities at listed nodes, the Float32 arrays of a box
// in VTK point order, and a non-finite / magnitude scan.  Every kernel takes its
// strides from Geo, so padded layouts work, and forms element offsets in 64 bits.
#include "observe.hpp"

#include <algorithm>
#include <cmath>

namespace gcmx {

namespace {

__device__ __forceinline__ double nt_load(const double* p) { return __builtin_nontemporal_load(p); }

// getQuantityOf at element offset `off`: the component, or the elastic PRESSURE
// with the host's roundings (trace = 0.0; trace += s_dd in order; -trace / D, a
// true division; 0.0 + -0.0 = +0.0 keeps the host's sign of zero).
template <bool NT>
__device__ __forceinline__ double observe_value(const double* __restrict__ cur, long long cs, long long off,
                                                int comp, const ObserveQ& oq) {
	if (comp != kObservePressure) return NT ? nt_load(cur + comp * cs + off) : cur[comp * cs + off];
	// all three loads are issued without a branch (diag[d] of an absent term is
	// component 0, its value is dropped), so that they overlap
	double trace = 0.0;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const double x = NT ? nt_load(cur + oq.diag[d] * cs + off) : cur[oq.diag[d] * cs + off];
		trace = d < oq.D ? trace + x : trace;
	}
	return -trace / (double)oq.D;
}

// One thread per (node, quantity); latency-bound.
__global__ __launch_bounds__(256) void k_gather_q(const double* __restrict__ cur, long long cs, long long n,
                                                  const long long* __restrict__ off, ObserveQ oq,
                                                  double* __restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * oq.n) return;
	const int k = (int)(i / n);
	const long long node = i - (long long)k * n;
	out[i] = observe_value<false>(cur, cs, off[node], oq.comp[k], oq);
}

// One thread per (receiver, quantity); latency-bound like k_gather_q.  K == 1 (a
// node recorder) stores observe_value itself, no multiply: the sample is bitwise
// k_gather_q's, the sign of zero and NaN payloads included.  K = 2^dim (a point
// recorder) blends the corners in ascending order, every product and sum rounded
// on its own (this file has the one exact build).
__global__ __launch_bounds__(256) void k_record(const double* __restrict__ cur, long long cs, long long n, int K,
                                                const long long* __restrict__ off, const double* __restrict__ wt,
                                                ObserveQ oq, double* __restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * oq.n) return;
	const int q = (int)(i / n);
	const long long r = i - (long long)q * n;
	const int comp = oq.comp[q];
	if (K == 1) {
		out[i] = observe_value<false>(cur, cs, off[r], comp, oq);
		return;
	}
	const long long* __restrict__ o = off + r * K;
	const double* __restrict__ w = wt + r * K;
	double acc = w[0] * observe_value<false>(cur, cs, o[0], comp, oq);
	for (int k = 1; k < K; k++) acc = acc + w[k] * observe_value<false>(cur, cs, o[k], comp, oq);
	out[i] = acc;
}

// The box of k_pack_vtk on the axes A (x: the VTK order's fastest), B (3-D: y) and
// F (the layer's fastest: z in 3-D, y in 2-D, stride 1).
// A strided launch (every stride-th node per axis) describes its lattice of
// output points with the same fields: na, nb, nf count output points, sa and sb
// are the element steps between selected rows (stride_a * Geo's, stride_b *
// Geo's), a0 = b0 = 0 with the box minimum of A and B folded into the kernel's
// `origin`, and f0 stays the first selected node of F; the step along F is the
// kernel's `xf`.
struct PackBox {
	int a0, b0, f0;    // box minimum (inner indices)
	int na, nb, nf;    // extents (nb = 1 below 3-D)
	long long sa, sb;  // element strides of A and B
	int ta, tf;        // tiles along A and F
};

// The transposition tile: kTile x kTile Float32, row = A index, column = F index.
// A load wave writes one row (consecutive dwords: conflict-free).  A store wave
// reads one column, lane l at row l: with the row stride = 3 (mod 32) the 32
// lanes of a half wave fall on 32 banks (3 is odd).  Velocity keeps three tiles
// whose stride is = 1 (mod 32): element e = 3 p + c of an output line reads
// tile c, row p, bank (c + 3 p + j) = (e + j) mod 32 -- consecutive lanes,
// consecutive banks.  17.2 KB per tile, 51.5 KB per block.
constexpr int kTile = 64;
constexpr int kTileRow = 67;
constexpr int kTileSize = kTile * kTileRow + 1;
static_assert(kTileRow % 32 == 3 && kTileSize % 32 == 1, "bank mapping of the tile");
constexpr int kPackBatch = 8;  // rows a wave loads before it converts and stores them to LDS

// One wave's 16 rows (w, w + 4, ...) of a tile, loaded kPackBatch at a time so that
// as many 512-byte loads are in flight per wave before the first conversion
// waits.  A row past the tile's last one reads that row again (a load without a
// branch; the stores never read it back).  PRESSURE: the elastic trace quantity,
// else component `comp`.
template <bool PRESSURE>
__device__ __forceinline__ void pack_load_tile(float* __restrict__ tile, const double* __restrict__ cur, long long cs,
                                               long long base, long long sa, int width, int w, int lane, int comp,
                                               const ObserveQ& oq) {
#pragma unroll
	for (int i0 = 0; i0 < kTile / 4; i0 += kPackBatch) {
		double v[kPackBatch];
		if constexpr (PRESSURE) {
			// every load of the batch first, then the traces (observe_value's arithmetic)
			double x[kPackBatch][3];
#pragma unroll
			for (int u = 0; u < kPackBatch; u++)
#pragma unroll
				for (int d = 0; d < 3; d++)
					x[u][d] = nt_load(cur + oq.diag[d] * cs + base + min(w + 4 * (i0 + u), width - 1) * sa);
#pragma unroll
			for (int u = 0; u < kPackBatch; u++) {
				double trace = 0.0;
#pragma unroll
				for (int d = 0; d < 3; d++) trace = d < oq.D ? trace + x[u][d] : trace;
				v[u] = -trace / (double)oq.D;
			}
		} else {
#pragma unroll
			for (int u = 0; u < kPackBatch; u++)
				v[u] = nt_load(cur + comp * cs + base + min(w + 4 * (i0 + u), width - 1) * sa);
		}
#pragma unroll
		for (int u = 0; u < kPackBatch; u++) tile[(w + 4 * (i0 + u)) * kTileRow + lane] = (float)v[u];
	}
}

// Block = one tile of one B index, four waves.  Loads: a wave reads 64
// consecutive F of one A index (512 B); the fp64 -> fp32 conversion (round to
// nearest even) happens before the LDS store.  Stores: a wave writes one (B, F)
// line of the output, 64 consecutive points (256 B per quantity, 768 B of
// Velocity as three instructions of 64 consecutive floats).
// STRIDED: the box is a lattice (PackBox) whose output column f is node f0 + f * xf
// of F, the layer's contiguous axis; only the load side's addressing differs.
// Lane l of a tile row's load reads column f_base + l, that is 8 bytes every xf
// elements: one instruction per row that touches 4 * xf lines of 128 B (64 at
// most), every one of them a line the lattice needs.  Whole-line loads with
// selection (xf coalesced 512-byte loads per row, a lane keeping the elements
// with f = f0 mod xf) fetch the same lines and measured the same within the
// spread at xf = 2, 4 and 8, so the simpler form is the one
// kept.  Rows and columns past the tile's edge are clamped in output indices, so
// a clamped load reads the last selected row or column, never a node outside the
// box.  The unit-stride instance ignores xf.
template <bool STRIDED>
__global__ __launch_bounds__(256) void k_pack_vtk(const double* __restrict__ cur, long long cs,
                                                  long long origin, int D, PackBox bx,
                                                  float* __restrict__ vel, ObserveQ oq,
                                                  float* __restrict__ qout, int xf) {
	__shared__ float tile[3 * kTileSize];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	long long t = blockIdx.x;
	const int a_base = (int)(t % bx.ta) * kTile;
	t /= bx.ta;
	const int f_base = (int)(t % bx.tf) * kTile;
	const int b = (int)(t / bx.tf);
	const int width = min(kTile, bx.na - a_base);   // A indices of this tile
	const int height = min(kTile, bx.nf - f_base);  // F indices of this tile
	const long long n_total = (long long)bx.na * bx.nb * bx.nf;
	// element offset of (a_base, b, f_base + lane); a lane past the tile's last column
	// reads that column again (a load without a branch; the stores never read it)
	long long base;
	if constexpr (STRIDED) {
		base = origin + (long long)a_base * bx.sa + (long long)b * bx.sb +
		       (bx.f0 + (long long)(f_base + min(lane, height - 1)) * xf);
	} else {
		base = origin + (long long)(bx.a0 + a_base) * bx.sa + (long long)(bx.b0 + b) * bx.sb +
		       (bx.f0 + f_base + min(lane, height - 1));
	}
	// first output point of line j of the tile: ((f * nb + b) * na + a_base)
	const long long line0 = ((long long)f_base * bx.nb + b) * bx.na + a_base;
	const long long line_step = (long long)bx.nb * bx.na;

	if (vel) {
		for (int c = 0; c < D; c++) pack_load_tile<false>(tile + c * kTileSize, cur, cs, base, bx.sa, width, w, lane, c, oq);
		__syncthreads();
		for (int j = w; j < height; j += 4) {
			float* dst = vel + 3 * (line0 + j * line_step);
#pragma unroll
			for (int k = 0; k < 3; k++) {
				const int e = lane + 64 * k;
				if (e < 3 * width) {
					const int p = e / 3, c = e - 3 * p;
					const float v = c < D ? tile[c * kTileSize + p * kTileRow + j] : 0.0f;
					__builtin_nontemporal_store(v, dst + e);
				}
			}
		}
		__syncthreads();
	}
	for (int k = 0; k < oq.n; k++) {
		// the quantity's kind is decided once per tile, outside the batched loads
		if (oq.comp[k] == kObservePressure) pack_load_tile<true>(tile, cur, cs, base, bx.sa, width, w, lane, 0, oq);
		else pack_load_tile<false>(tile, cur, cs, base, bx.sa, width, w, lane, oq.comp[k], oq);
		__syncthreads();
		float* dst = qout + k * n_total;
		for (int j = w; j < height; j += 4)
			if (lane < width) __builtin_nontemporal_store(tile[lane * kTileRow + j], dst + line0 + j * line_step + lane);
		__syncthreads();
	}
}

// 1-D: the layer's order is the VTK order; one thread per output point (node
// a0 + i * xa).
__global__ __launch_bounds__(256) void k_pack_line(const double* __restrict__ cur, long long cs, long long origin,
                                                   int a0, int na, int xa, float* __restrict__ vel, ObserveQ oq,
                                                   float* __restrict__ qout) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= na) return;
	const long long off = origin + a0 + (long long)i * xa;
	if (vel) {
		vel[3 * (long long)i] = (float)cur[off];
		vel[3 * (long long)i + 1] = 0.0f;
		vel[3 * (long long)i + 2] = 0.0f;
	}
	for (int k = 0; k < oq.n; k++) qout[(long long)k * na + i] = (float)observe_value<false>(cur, cs, off, oq.comp[k], oq);
}

// Health check over the inner nodes.  A work item is one segment (kScanSeg
// elements) of one row of the fastest axis; a wave takes items in a grid stride
// and its lanes consecutive elements.  Count and maxima do not depend on the
// order they are combined in: wave shuffles, LDS across the four waves, then one
// atomic per block and word (the maxima as the bit patterns of non-negative
// doubles, which order like the values).
constexpr int kScanSeg = 4096;
__global__ __launch_bounds__(256) void k_scan(const double* __restrict__ cur, long long cs, long long origin, int M,
                                              int nF, int nB, long long sA, long long sB, long long items,
                                              int nseg, unsigned long long* __restrict__ res) {
	__shared__ unsigned long long part[4][kScanWords];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	double mx[kMaxM];
#pragma unroll
	for (int c = 0; c < kMaxM; c++) mx[c] = 0.0;
	unsigned long long bad = 0;
	const long long nwaves = (long long)gridDim.x * 4;
	for (long long item = (long long)blockIdx.x * 4 + w; item < items; item += nwaves) {
		const long long row = item / nseg;
		const int seg = (int)(item - row * nseg);
		const long long a = row / nB, b = row - a * nB;
		const long long base = origin + a * sA + b * sB;
		const int f_end = min(nF, (seg + 1) * kScanSeg);
		for (int f = seg * kScanSeg + lane; f < f_end; f += 64) {
#pragma unroll
			for (int c = 0; c < kMaxM; c++)
				if (c < M) {
					const double av = fabs(nt_load(cur + c * cs + base + f));
					if (av < __builtin_inf()) mx[c] = fmax(mx[c], av);  // false for NaN and Inf
					else bad++;
				}
		}
	}
	for (int d = 32; d > 0; d >>= 1) {
		bad += __shfl_down(bad, d);
#pragma unroll
		for (int c = 0; c < kMaxM; c++) mx[c] = fmax(mx[c], __shfl_down(mx[c], d));
	}
	if (lane == 0) {
		part[w][0] = bad;
#pragma unroll
		for (int c = 0; c < kMaxM; c++) part[w][1 + c] = (unsigned long long)__double_as_longlong(mx[c]);
	}
	__syncthreads();
	const int k = threadIdx.x;
	if (k == 0) {
		const unsigned long long s = part[0][0] + part[1][0] + part[2][0] + part[3][0];
		if (s) atomicAdd(&res[0], s);
	} else if (k <= M) {
		const unsigned long long m = max(max(part[0][k], part[1][k]), max(part[2][k], part[3][k]));
		if (m) atomicMax(&res[k], m);
	}
}

}  // namespace

void launch_gather_q(const double* cur, const Geo& g, long long n, const long long* off_d, const ObserveQ& oq,
                     double* out_d, hipStream_t st) {
	const long long total = n * oq.n;
	if (total <= 0) return;
	hipLaunchKernelGGL(k_gather_q, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cur, g.cs, n, off_d, oq,
	                   out_d);
}

void launch_record(const double* cur, const Geo& g, long long n, int K, const long long* off_d, const double* w_d,
                   const ObserveQ& oq, double* out_d, hipStream_t st) {
	const long long total = n * oq.n;
	if (total <= 0) return;
	hipLaunchKernelGGL(k_record, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cur, g.cs, n, K, off_d, w_d,
	                   oq, out_d);
}

void launch_pack_vtk(const double* cur, const Geo& g, const int bmin[3], const int bmax[3], float* vel_d,
                     const ObserveQ& oq, float* q_d, hipStream_t st) {
	if (g.D == 1) {
		const int na = bmax[0] - bmin[0];
		hipLaunchKernelGGL(k_pack_line, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, cur, g.cs, g.origin,
		                   bmin[0], na, 1, vel_d, oq, q_d);
		return;
	}
	const int F = g.D - 1;
	PackBox bx;
	bx.a0 = bmin[0];
	bx.na = bmax[0] - bmin[0];
	bx.b0 = g.D == 3 ? bmin[1] : 0;
	bx.nb = g.D == 3 ? bmax[1] - bmin[1] : 1;
	bx.f0 = bmin[F];
	bx.nf = bmax[F] - bmin[F];
	bx.sa = g.stride[0];
	bx.sb = g.D == 3 ? g.stride[1] : 0;
	bx.ta = (bx.na + kTile - 1) / kTile;
	bx.tf = (bx.nf + kTile - 1) / kTile;
	const long long blocks = (long long)bx.ta * bx.tf * bx.nb;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack_vtk<false>), dim3((unsigned)blocks), dim3(256), 0, st, cur, g.cs,
	                   g.origin, g.D, bx, vel_d, oq, q_d, 1);
}

void launch_pack_vtk_strided(const double* cur, const Geo& g, const int bmin[3], const int n[3], const int step[3],
                             float* vel_d, const ObserveQ& oq, float* q_d, hipStream_t st) {
	if (g.D == 1) {
		hipLaunchKernelGGL(k_pack_line, dim3((unsigned)((n[0] + 255) / 256)), dim3(256), 0, st, cur, g.cs, g.origin,
		                   bmin[0], n[0], step[0], vel_d, oq, q_d);
		return;
	}
	const int F = g.D - 1;
	PackBox bx;
	bx.a0 = bx.b0 = 0;
	bx.na = n[0];
	bx.nb = g.D == 3 ? n[1] : 1;
	bx.f0 = bmin[F];
	bx.nf = n[F];
	bx.sa = (long long)step[0] * g.stride[0];
	bx.sb = g.D == 3 ? (long long)step[1] * g.stride[1] : 0;
	bx.ta = (bx.na + kTile - 1) / kTile;
	bx.tf = (bx.nf + kTile - 1) / kTile;
	const long long origin = g.origin + (long long)bmin[0] * g.stride[0] + (g.D == 3 ? (long long)bmin[1] * g.stride[1] : 0);
	const long long blocks = (long long)bx.ta * bx.tf * bx.nb;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack_vtk<true>), dim3((unsigned)blocks), dim3(256), 0, st, cur, g.cs, origin,
	                   g.D, bx, vel_d, oq, q_d, step[F]);
}

double pack_strided_traffic(const Geo& g, const int n[3], const int step[3], double planes, double out_bytes) {
	const int F = g.D - 1;
	const double rows = g.D == 1 ? 1.0 : (double)n[0] * (g.D == 3 ? n[1] : 1);
	const double span_lines = std::ceil((((double)n[F] - 1) * step[F] + 1) * sizeof(double) / 128.0);
	return rows * planes * std::min(span_lines, (double)n[F]) * 128.0 + out_bytes;
}

void launch_scan(const double* cur, const Geo& g, unsigned long long* res_d, hipStream_t st) {
	(void)hipMemsetAsync(res_d, 0, kScanWords * sizeof(unsigned long long), st);
	const int F = g.D - 1;
	const int nF = g.sizes[F];
	const int nB = g.D == 3 ? g.sizes[1] : 1;
	const long long nA = g.D >= 2 ? g.sizes[0] : 1;
	const long long sA = g.D >= 2 ? g.stride[0] : 0, sB = g.D == 3 ? g.stride[1] : 0;
	const int nseg = (nF + kScanSeg - 1) / kScanSeg;
	const long long items = nA * nB * nseg;
	const long long blocks = std::min<long long>((items + 3) / 4, 2048);
	hipLaunchKernelGGL(k_scan, dim3((unsigned)blocks), dim3(256), 0, st, cur, g.cs, g.origin, g.M, nF, nB, sA, sB,
	                   items, nseg, res_d);
}

}  // namespace gcmx
