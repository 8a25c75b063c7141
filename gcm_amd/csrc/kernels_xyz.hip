// kernels_xyz.hip -- the one-pass 3-D time step of the isotropic medium (X, Y
// and Z stages of cubic::Engine::nextTimeStep, Engine.cpp:90-121, fused into one
// kernel): k_step_tx2 with its z-seam kernel (below), the one-plane kernel
// (plane_step.hpp) for what k_step_tx2 does not take, and their launcher.
// Arithmetic identical to k_stage_generic / the reference stage
// (engine/cubic/GridCharacteristicMethod.hpp:42-52) through node_update (iso.hpp).
#include "iso.hpp"

#include <cstring>
#include <string>
#include <type_traits>

// This file is compiled twice (Makefile): as the exact build (xyz_exact,
// -ffp-contract=off: the reference's separate multiply and add roundings,
// bitwise equal to the oracle) and as the FMA build (xyz_fma, -DGCMX_FMA=1
// -ffp-contract=fast: multiply-adds contracted, within the north-star fp64
// tolerance of the reference).  gcmx_set_fp_mode selects one.
#ifndef GCMX_FMA
#define GCMX_FMA 0
#endif
#if GCMX_FMA
#define GCMX_BUILD_NS xyz_fma
#define GCMX_FP_TAG ", FMA"
#else
#define GCMX_BUILD_NS xyz_exact
#define GCMX_FP_TAG ""
#endif
#include "plane_step.hpp"

namespace gcmx {
namespace GCMX_BUILD_NS {

// k_step_tx2 (below) takes every launch with borderSize <= 2 and Z <= 512; the
// one-plane kernel (reported as k_fused_xyz) runs borderSize 3 and the rows of
// 513 .. 1024 the z split does not take.

// ------------------------------------------------ two planes per thread --

constexpr int kTx2MinWaves = 2;  // waves per SIMD (<= 256 VGPRs): one 512-lane block per CU
// Old blocks' share of two generations' rows, percent (tx2_gen2; the runtime
// variable GCMX_TX2_GEN2 overrides it, 0: off).  256^3: 0.530-0.540 against
// 0.547-0.559 ms off, profiles/r6/s
constexpr int kTx2Gen2Default = 64;
#ifndef GCMX_TX2_BLKT  // tuning builds only: per-wave start / end times (s_memrealtime, 100 MHz) and the
#define GCMX_TX2_BLKT 0  // CU of every block of the last k_step_tx2 launch (gcmx_diag_blk*)
#endif
#if GCMX_TX2_BLKT
constexpr int kBlkMax = 8192;
__device__ unsigned long long g_tx2_blk[kBlkMax][8][2];  // [block][wave][start, end]
__device__ unsigned g_tx2_hw[kBlkMax];                   // HW_ID of the block's wave 0
#endif


// Per-node materials: every lane applies ITS OWN material's table, read from
// the LDS copy with a per-lane address.  (Rounds 3-4 wrapped this in a
// readfirstlane "waterfall" loop, `for (;;) { k = readfirstlane(key); if (key
// == k) { f(k); break; } }`, meant to keep k wave-uniform.  Inside `key == k`
// the compiler replaces k by the lane's own key, after which the loop carries
// nothing uniform and is deleted: every lane runs f once with its own key, all
// lanes active.  With tables read per lane that is still correct (and is what
// the shipped round-4 ISA does: ds_read at a per-lane address, no loop); the
// mid-round-4 variant that also passed the table fields through readfirstlane
// (cb6938f) then broadcast the FIRST lane's table to the whole wave -- wrong
// for every lane of another material (relative L2 0.687 on random material
// ids, green on layered ids where a wave holds one material).  DESIGN.md §3.1.)

// Component held in window slot q of a stage whose window mask is `mask`.
__host__ __device__ constexpr int wcomp(unsigned mask, int q) {
	int n = 0;
	for (int j = 0; j < 9; j++)
		if ((mask >> j) & 1u) {
			if (n == q) return j;
			n++;
		}
	return -1;
}

// The whole time step in one pass with TWO adjacent x planes per thread
// (x, x+1 at one z) -- the default 3-D step for borderSize <= 2, Z <= 512.
//
// Why two planes: the X stages of both nodes read the 2*BS+2 planes
// x-BS .. x+1+BS, i.e. 6*(2*BS+2) + 2*3 loads per two nodes instead of
// 2*(6*(2*BS+1) + 3).  Those x-neighbour re-reads are L2->CU traffic, and that
// traffic, not HBM, bounds the one-plane kernel: tools/xyz_probe.hip measures the
// bare access pattern at 33 loads + 9 stores per node 1.35x slower than the
// compulsory 9 + 9, and at two planes per thread 1.12x.
//
// Arithmetic per node is k_fused_xyz's (pair_update / node_update, reference
// operation order), except that with floor(q) == 0 the X stage's Newton
// differences are shared by the two nodes: with forward differences along x,
//   D0_k = S_k,  Di_k = (D(i-1)_{k+1} - D(i-1)_k) * c_{i-1},
// the +x foot of node m interpolates (S_m + D1_m) + D2_m ... exactly as
// minMaxInterpolate does (EqualDistanceLineInterpolator.hpp:56-71), and the -x
// foot, whose values are S_m, S_{m-1}, ..., has d_i = (-1)^i Di_{m-i}, so
// (S_m - D1_{m-1}) + D2_{m-2} ...: a - b == -(b - a) and (-x) * c == -(x * c)
// in IEEE arithmetic, up to the sign of an exact zero (IEEE-equal, DESIGN.md
// §3.2).  The -x limiter bounds of node x+1 are the +x bounds of node x.
//
// Schedule (each choice measured A/B on MI355X): registers hold
// the two Y windows; the node-only Y components of rows y..y+BS (read back by
// the same thread only) live in an LDS ring.  The Y results reach the Z stage in
// one of two ways.  UNI instances (Z == ZT, whole waves): every wave keeps its
// 64 columns in a region of its own, only the BS edge values per side cross to
// the neighbour waves through a two-row edge ring, and a per-wave row counter
// says which rows are there -- no block barrier, so the waves of a block drift
// apart and overlap their memory phases.  !UNI instances: one block buffer per
// node between two barriers per row.  Loads of the next row: the UNI instances
// issue its first two pairs before the Z stage; the !UNI instances issue the
// first pair there and the second between the two nodes' Z stages.  Each node's
// 9 stores follow its own Z stage (16-byte path: both nodes' after the second);
// the last pair and the node-only loads are issued when the X stage starts.
// One 512-thread block per CU (2 waves/SIMD, <= 256 VGPRs).  Loads and stores
// are buffer-style: SGPR plane bases, block-uniform offsets, one 32-bit per-lane
// byte offset; the new layer is written with non-temporal stores.
//
// FACES: uniform cubic border conditions on the y/z faces (FaceBC): the ghost
// rows of the Y stage and the ghost columns of the Z stage are the mirrored
// inner X / Y results with the overridden components set to -inner + 2 f(t)
// (BorderConditions.hpp:94-114, applied to the intermediate layers as
// Engine::nextTimeStep does before each stage, Engine.cpp:90-121).  Only the
// window components of those ghosts are ever read, so they are all that is
// formed.  Requires Y, Z >= 2*BS+2 (the mirrored rows are inner rows) and no
// PRESSURE condition on a y/z face (its trace needs the node-only components);
// x faces are filled in memory before the launch (k_face_fill).
// Without FACES, y/z ghosts of both layers must be zero.
//
// If the launch has an odd number of planes the last thread's second node is
// computed from clamped (valid) planes and not stored.
//
// HET: per-node materials (heterogeneous media, TestEngine.cpp:139-296's layers).
// Every node's stages use its own material's tables mtab[mat[node]] (per material
// the three axes' tables are identical and floor(q) = 0, checked on the host), as
// GridCharacteristicMethod::stage takes each node's own matrices.  The tables are
// read per lane from their LDS copy; where the two nodes of a lane differ in
// material, their X stages run without the shared differences (pair_update per
// node).
//
// ZS (z split, Z = nz * ZT > 512, uniform medium, no faces): a z row no longer
// fits one block's register windows (two planes x 1024 z x 6 components x 5 rows
// of fp64 = 94 % of a CU's register file), so each row is cut into nz parts of
// ZT lanes, one block each.  A part's Z stage is exact except in the BS lanes
// next to a cut, which need the other part's Y results: those lanes do not
// store, and k_zseam recomputes the X and Y stages of the 4*BS columns around
// each cut and stores their Z stage after the launch (1024^3: 8 of 1024 columns).
// (Handing the cut lanes' Y results over through memory instead cost 25 %: those
// lanes' extra stores sit in the vmcnt queue the row-ahead loads are waited on
// with, profiles/r6/h.)
template <int BS, int ZT, bool KF0, bool UNI, bool FACES, bool HET, bool ZS = false, bool WD = false>
__global__ __launch_bounds__(ZT, kTx2MinWaves) void k_step_tx2(
    const double* __restrict__ in, double* __restrict__ outl, Geo g, IsoAxis AX, IsoAxis AY_,
    IsoAxis AZ_, int x0, int chunk, int nplanes, int xb0, int nplanesb, FaceBC fb,
    const IsoAxis* __restrict__ mtab, const uint8_t* __restrict__ mat) {
	static_assert(!HET || (KF0 && UNI), "heterogeneous step: floor(q) = 0, Z == ZT, equal axes");
	static_assert(!ZS || (UNI && !HET), "z split: uniform medium");
	const IsoAxis& AY = UNI ? AX : AY_;
	const IsoAxis& AZ = UNI ? AX : AZ_;
	constexpr unsigned WMX = iso_window(0);
	constexpr unsigned CMX = iso_center_only(0);
	constexpr int NCX = popc9(CMX);
	constexpr unsigned WMY = iso_window(1);
	constexpr unsigned CMY = iso_center_only(1);
	constexpr int NWY = popc9(WMY);
	constexpr int NCY = popc9(CMY);
	constexpr unsigned WMZ = iso_window(2);
	constexpr int NWZ = popc9(WMZ);
	constexpr int W = 2 * BS + 1;
	constexpr int WX = W + 1;  // planes x-BS .. x+1+BS
	constexpr int LW = ZT + 2 * BS;
	static_assert(NCX >= 1 && NCY >= 1, "isotropic structure");
	// NB (every UNI instance): Z == ZT, a multiple of 64.  Each wave keeps its own Y
	// results in a region of 64 + 2 BS slots; only the BS edge values per side cross
	// to the neighbour waves, through a two-row ring `eg` and a per-wave row counter
	// `rdy` (no block barrier: the waves of a block drift apart and overlap their
	// memory phases).  The !UNI instances exchange through `zl` between barriers.
	constexpr bool NB = UNI;
	constexpr int NW = ZT / 64;
	static_assert(!NB || ZT % 64 == 0, "NB needs whole waves");
	// WIDE: the instance's WD argument, which only barrier-free (UNI) instances
	// may set.  The launcher sets it where every plane, row and part of the launch
	// starts 16-byte aligned (tx2_wide_ok) and the instance gains from it (go_uni).
	// Lane l < 32 of a wave owns column 2l of the wave's 64-column block and lane
	// l + 32 column 2l + 1, so one 16-byte access of lane l covers the columns of
	// lanes l and l + 32.  A load brings those two columns of ONE plane -- the
	// lower half-wave addresses plane a, the upper half plane b -- and half_swap
	// turns the two halves' pairs into every lane's own column of planes a and b;
	// stores run the same exchange backwards.  `z`, `ln`, `wv` keep their meaning
	// (the lane's column); only the LDS slots are by lane.
	constexpr bool WIDE = WD && NB;
	static_assert(!WD || WIDE, "wide instance needs the barrier-free exchange (UNI)");
	// WIDE: a wave's region holds its even columns -2 .. 64 in slots 0 .. 33 and
	// its odd columns -1 .. 65 in slots 34 .. 67 (each half-wave reads and writes
	// 32 consecutive slots: no bank conflicts, as 64 consecutive ones by z)
	constexpr int RW = WIDE ? 68 : 64 + 2 * BS;
	// the barrier instances split the ahead-loads around the two nodes' Z stage + stores
	constexpr bool ZS2 = !NB;
	__shared__ double zl[NB ? 1 : 2][NB ? 1 : NWZ][NB ? 1 : LW];  // Y results of both nodes (Z stage input)
	__shared__ double rg[NB ? NW : 1][NB ? 2 : 1][NB ? NWZ : 1][NB ? RW : 1];
	__shared__ double eg[NB ? 2 : 1][NB ? NW : 1][2][NB ? 2 : 1][NB ? NWZ : 1][BS];  // [row&1][wave][side][node][comp][k]
	__shared__ int rdy[NB ? NW : 1];                                               // last row whose edges are in eg
	__shared__ double cl[BS + 1][2][NCY][ZT];  // node-only Y components, rows y..y+BS (ring)
	// HET: every material's tables in LDS (<= kHetMaxMaterials, host-checked).  A
	// global (or flat: LDS-or-global) table load in the row loop would count in
	// vmcnt, and waiting for it would wait for every row-ahead load issued before
	// it -- the software pipeline collapses (measured: HET 256^3 +34 %).
	__shared__ IsoAxis hlds[HET ? kHetMaxMaterials : 1];
	__shared__ double hode[HET ? kHetMaxMaterials : 1];  // HET: folded ODE factor per material

	// z blocks of 64 columns dealt so that the two waves sharing a SIMD (w and
	// w + 4 of a 512-lane block) hold neighbouring z blocks 2w and 2w + 1
	// (512^3: 3.548-3.570 against 3.572-3.589 ms in block order, profiles/r6/w)
	const int z = [] {
		int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		if constexpr (ZT == 512) w = w < 4 ? 2 * w : 2 * (w - 4) + 1;
		const int l = (int)(threadIdx.x & 63);
		return w * 64 + (WIDE ? ((l & 31) << 1) | (l >> 5) : l);
	}();
#if GCMX_TX2_BLKT
	const unsigned long long blk_t0_ = __builtin_amdgcn_s_memrealtime();
#endif
	const int Y = g.sizes[1], Z = g.sizes[2];
	int x, yb, ye, xbeg, xend;
	bool rev;  // this block marches its rows downwards (odd chunks, see `run`)
	int zp = 0;                                    // ZS: this block's part of the z row
	const int nz = ZS ? g.sizes[2] / ZT : 1;
	{  // XCD-aware chunk-major block order (see k_fused_xyz) over the plane pairs of
	   // range A [x0, x0 + nplanes), then range B [xb0, xb0 + nplanesb) (may be empty).
	   // Pairs are GLOBAL: (2k, 2k+1) in the global x index g.gx0 + x, so a range
	   // starting at an odd global plane begins with a pair whose first node is not
	   // ours.  The two nodes of a pair run different (contracted, in the FMA build)
	   // operation sequences, so global pairing keeps every node's sequence, and with
	   // it every bit, independent of how the grid is cut into slabs or bodies.
		const int pa = (g.gx0 + x0) & 1, pb = (g.gx0 + xb0) & 1;
		const int npa = (nplanes + pa + 1) / 2;
		const int npair = npa + (nplanesb > 0 ? (nplanesb + pb + 1) / 2 : 0);
		const int T = (int)gridDim.x, b = (int)blockIdx.x;
		const int p = xcd_order(b, T);
		int q = p % npair;
		int cidx = p / npair;  // chunk index
		if (!ZS && chunk < 0) {
			// Two generations (tx2_gen2): the launch is exactly two resident blocks per
			// CU, and the first block dispatched to a CU (blocks [0, T/2)) runs ahead of
			// its younger neighbour (oldest-first issue): old blocks take chunks of
			// `co` rows, young ones `cy`.  Per generation, XCD k's blocks take the
			// k-th contiguous run of (pair, chunk slot s) positions, pairs fastest;
			// an old block runs chunk s, a young one chunk ncg + s.
			const int co = (-chunk) & 0xFFFF, half = T >> 4;
			const int j = b >> 3, gen = j >= half ? 1 : 0;
			const int G = (b & 7) * half + (j - gen * half);
			const int ncg = (T >> 1) / npair;  // chunks per generation
			q = G % npair;
			cidx = G / npair + gen * ncg;
			const int cy = (-chunk) >> 16;
			auto start = [&](int c) { return c <= ncg ? c * co : ncg * co + (c - ncg) * cy; };
			yb = start(cidx);
			ye = min(start(cidx + 1), Y);  // the host makes ncg (co + cy) == Y
		}
		x = q < npa ? x0 - pa + 2 * q : xb0 - pb + 2 * (q - npa);
		xbeg = q < npa ? x0 : xb0;
		xend = q < npa ? x0 + nplanes : xb0 + nplanesb;
		// ZS: pairs fastest, then parts, then chunks.  An XCD's concurrent blocks then
		// cover twice the consecutive pairs of an order with the parts of a pair
		// adjacent: 1024^3 -1.2 % (profiles/r6/n)
		if constexpr (ZS) {
			zp = cidx % nz;
			cidx /= nz;
		}
		if (ZS || chunk > 0) {
			yb = cidx * chunk;
			ye = min(yb + chunk, Y);
		}
		rev = cidx & 1;
	}
	const bool one = x >= xbeg;  // node x is ours (else only x + 1 is)
	const bool two = x + 1 < xend;
	const bool live = UNI || z < Z;
	const int zc = live ? z : Z - 1;
	const unsigned stx = (unsigned)g.stride[0];
	const unsigned sty = (unsigned)g.stride[1];
	// plane bases at this block's plane x (SGPRs), offsets relative to them:
	// 32-bit whatever the layer's size (onepass_layout_ok)
	const long long pbase = (long long)x * g.stride[0];
	const unsigned plane = (unsigned)g.origin;  // node (x, 0, 0) from the bases
	const unsigned zo = live ? (unsigned)z : (unsigned)Z;
	// Memory accessors.  ldx(j, k, r): component j of plane x - BS + k (the last
	// plane clamped when x + 1 is not ours), row r, this lane's column;
	// stz(c, t, y, v): component c of node (x + t, y) of the output layer.
	// Buffer-style: block-uniform offsets in SGPRs, no VALU address math.
	const Planes src(in + pbase, g.cs);
	const PlanesW out_p(outl + pbase, g.cs);
	const unsigned zpart = ZS ? (unsigned)(zp * ZT) : 0u;      // ZS: first column of this part
	const int zg = (int)zpart + zc;                            // the lane's column in the row
	const unsigned lv = (zpart + (unsigned)zc) * 8u, sv = (zpart + zo) * 8u;  // per-lane byte offsets
	const unsigned pxm = plane - (unsigned)BS * stx;      // plane x - BS, row 0, column 0
	auto ldx = [&](int j, int k, int r) {
		// planes outside the valid range (x - BS when x is not ours, x + 1 + BS when
		// x + 1 is not ours) are read by the discarded node only: clamp them
		const int d = (k == WX - 1 && !two) ? 2 * BS : (k == 0 && !one) ? 1 : k;
		return ld_b(src, j, opaque_u32(lv + (pxm + (unsigned)d * stx + (unsigned)r * sty) * 8u));
	};
	// the node-only components of the own planes: read once, by this lane only,
	// so by non-temporal loads (+0.4 % against plain ones, profiles/r4/ab)
	auto ldc = [&](int j, int k, int r) {
		const int d = (k == WX - 1 && !two) ? 2 * BS : (k == 0 && !one) ? 1 : k;
		return ld_nt_b(src, j, opaque_u32(lv + (pxm + (unsigned)d * stx + (unsigned)r * sty) * 8u));
	};
	auto stz = [&](int c, int t, int y, double v) {  // non-temporal, as every store of the new layer
		st_nt_b(out_p, c, opaque_u32(sv + (plane + (unsigned)t * stx + (unsigned)y * sty) * 8u), v);
	};
	// WIDE accessors.  ldw(j, ka, kb, r): the lane's 16 bytes (columns 2l, 2l + 1 of
	// its wave's block) of component j, row r, of window plane ka (lower half-wave)
	// or kb (upper half), clamped like ldx's; half_swap(v.x, v.y) after the wait
	// makes them the lane's own column of planes ka and kb.  stw: the reverse, node
	// x from the lower half-wave and node x + 1 from the upper.
	const bool hsel = (threadIdx.x & 32u) != 0;  // upper half-wave
	const unsigned lw = (zpart + (unsigned)(z & ~63) + 2u * (threadIdx.x & 31u)) * 8u;
	auto ldw = [&](int j, int ka, int kb, int r, bool nt) {
		auto cl_ = [&](int k) { return (k == WX - 1 && !two) ? 2 * BS : (k == 0 && !one) ? 1 : k; };
		const unsigned pa = (pxm + (unsigned)cl_(ka) * stx) * 8u, pb = (pxm + (unsigned)cl_(kb) * stx) * 8u;
		const unsigned o = opaque_u32(lw + (hsel ? pb : pa) + (unsigned)r * sty * 8u);
		return nt ? ld2_nt_b(src, j, o) : ld2_b(src, j, o);
	};
	auto stw = [&](int c, int y, double v0, double v1) {
		const unsigned o = opaque_u32(lw + (plane + (hsel ? stx : 0u) + (unsigned)y * sty) * 8u);
		const dpair v = {v0, v1};
		st2_nt_b(out_p, c, o, v);
	};
	// per-material table k (the lane's own material), from the LDS copy made at
	// kernel start.  Measured alternatives: scalar loads through
	// the constant address space spill VGPRs; separate one-table / two-table X
	// paths double the X stage's code; both are slower.
	auto mt = [&](unsigned k) -> const IsoAxis& { return hlds[k]; };
	// (a lambda on purpose: with ghost_rule reading fb.two_v directly the FACES
	// instances come out with other SGPR spill counts, i.e. other instructions)
	auto two_v = [&](int f, int j) -> double { return fb.two_v[f][j]; };
	// The condition of face f at node x + t (pos = the node's z on y faces, its y
	// on z faces), resolved once per node: the overridden components and their
	// 2 f(t) (components in `need` only).  A face with a per-node map (partial
	// faces) takes the face node's own condition; none: the ghost stays 0.
	struct GhostRule {
		unsigned mask;
		bool none;
		double two[9];
	};
	auto ghost_rule = [&](int f, int t, int pos, unsigned need) -> GhostRule {
		GhostRule r;
		r.none = false;
		if (fb.map[f]) {
			const int xx = (t == 1 && !two) ? x : (t == 0 && !one) ? x + 1 : x + t;
			const unsigned c = fb.map[f][(size_t)xx * (f < 2 ? Z : Y) + pos];
			r.none = c == kNoFaceCond;
			const FaceCond& fc = fb.conds[r.none ? 0u : c];
			r.mask = r.none ? 0u : fc.mask;
#pragma unroll
			for (int j = 0; j < 9; j++)
				if ((need >> j) & 1u) r.two[j] = r.none ? 0.0 : fc.two_v[j];
		} else {
			r.mask = fb.mask[f];
#pragma unroll
			for (int j = 0; j < 9; j++)
				if ((need >> j) & 1u) r.two[j] = two_v(f, j);
		}
		return r;
	};
	// ghost value of component j: -inner + 2 f(t) if overridden, else the mirror
	auto ghost = [](const GhostRule& r, int j, double v) -> double {
		return r.none ? 0.0 : ((r.mask >> j) & 1u) ? -v + r.two[j] : v;
	};

	const int wv = z >> 6, ln = z & 63;  // wave in block, lane
	// ZS: lanes whose Z stage needs the neighbouring part (k_zseam stores them)
	const bool seam_own = ZS && ((zp > 0 && z < BS) || (zp < nz - 1 && z >= ZT - BS));
	// NB: slot of column c (-BS .. 63 + BS of the wave's block) in the wave's region
	auto rs = [](int c) { return WIDE ? (c >> 1) + ((c & 1) ? 35 : 1) : BS + c; };
	// the lane's own slot and its z + 1 neighbour's: the Z stage's neighbours at
	// distance o sit at constant offsets from one of the two (WIDE: odd distances
	// in the other parity's run, even ones in the lane's own)
	const int rs0 = rs(ln), rs1 = rs(ln + 1);
	auto rso = [&](int o) { return !WIDE ? rs0 + o : (o & 1) ? rs1 + ((o - 1) >> 1) : rs0 + (o >> 1); };
	// WIDE: the lane's 16-byte store covers columns cb, cb + 1 of its part; it is
	// left out only where k_zseam writes both (a part's cut lanes still compute;
	// with BS = 1 the pair at a cut holds one cut column, stored here and then
	// overwritten by k_zseam, which runs after this launch on the same stream)
	const bool seam_pair = [&] {
		const int cb = (z & ~63) + 2 * (int)(threadIdx.x & 31u);
		auto sc = [&](int c) { return (zp > 0 && c < BS) || (zp < nz - 1 && c >= ZT - BS); };
		return ZS && sc(cb) && sc(cb + 1);
	}();
	const int ci = WIDE ? (int)threadIdx.x : z;  // the lane's slot in the `cl` ring (read back by itself only)
	// NB: the hand-over lanes of `collect`.  A side of a wave's ring row is NE
	// contiguous values [node t][component q][k]; HARDWARE lane e < NE of the lower
	// half-wave takes value e of the left neighbour's right side, lane 32 + e value
	// e of the right neighbour's left side, each into the own halo slot of column
	// k - BS (left) or 64 + k (right).  Wave 0 has no left and wave NW - 1 no right
	// neighbour: those halo slots keep their zeros or publish's face ghosts, and no
	// lane of that half copies.  Both places are fixed for the launch and share one
	// register (the row loop has none to spare): `hpk` = the element of ring row 0
	// in `eg` (collect adds the row) in the low half, the element of `rg` in the
	// high half; sign bit set: the lane does not copy.
	constexpr int NE = 2 * NWZ * BS;  // edge values per side
	constexpr int ESZ = NW * 2 * NE;  // doubles per ring row
	static_assert(!NB || NE <= 32, "one edge value per lane of a half-wave");
	static_assert(!NB || (2 * ESZ <= 0x10000 && NW * 2 * NWZ * RW <= 0x8000), "hpk: 16 + 15 bits");
	unsigned hpk = ~0u;
	if constexpr (NB && NW > 1) {
		const int e = (int)(threadIdx.x & 31u);
		const bool right = (threadIdx.x & 32u) != 0;
		if (e < NE && (right ? wv < NW - 1 : wv > 0)) {
			const int k = e % BS, q = (e / BS) % NWZ, t = e / (BS * NWZ);
			const int src = ((right ? wv + 1 : wv - 1) * 2 + (right ? 0 : 1)) * NE + e;
			const int dst = ((wv * 2 + t) * NWZ + q) * RW + rs(right ? 64 + k : k - BS);
			hpk = (unsigned)src | ((unsigned)dst << 16);
		}
	}
	if constexpr (NB) {  // zero halos (z ghosts stay zero without a z face); counters
		if (ln < BS || ln >= 64 - BS) {
			const int hs = rs(ln < BS ? ln - BS : ln + BS);
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int q = 0; q < NWZ; q++) rg[wv][t][q][hs] = 0.0;
		}
		if (z < NW) rdy[z] = -1;  // rows published, counted in marching order
		__syncthreads();
	} else if (z < 2 * BS) {
		const int gslot = (z < BS) ? z : (Z + z);
#pragma unroll
		for (int t = 0; t < 2; t++)
#pragma unroll
			for (int q = 0; q < NWZ; q++) zl[t][q][gslot] = 0.0;
	}

	typedef double PairWin[2][WX];  // [vel/sig][plane]
	auto pair_load = [&](auto PC, PairWin& w, int r) {
		constexpr int P = decltype(PC)::value;
		if constexpr (WIDE) {  // raw half-wave pairs: pair_fix before use
#pragma unroll
			for (int m = 0; m < WX / 2; m++) {
				const dpair a = ldw(pair_vel(0, P), 2 * m, 2 * m + 1, r, false);
				const dpair b = ldw(pair_sig(0, P), 2 * m, 2 * m + 1, r, false);
				w[0][2 * m] = a.x, w[0][2 * m + 1] = a.y;
				w[1][2 * m] = b.x, w[1][2 * m + 1] = b.y;
			}
			return;
		}
#pragma unroll
		for (int k = 0; k < WX; k++) {
			w[0][k] = ldx(pair_vel(0, P), k, r);
			w[1][k] = ldx(pair_sig(0, P), k, r);
		}
	};
	// WIDE: a loaded pair window, once its loads have landed, into the lane's own column
	auto pair_fix = [&](const PairWin& w, PairWin& u) {
#pragma unroll
		for (int v = 0; v < 2; v++) {
#pragma unroll
			for (int k = 0; k < WX; k++) u[v][k] = w[v][k];
			if constexpr (WIDE) {
#pragma unroll
				for (int m = 0; m < WX / 2; m++) half_swap(u[v][2 * m], u[v][2 * m + 1]);
			}
		}
	};
	// Rows 2P, 2P+1 of r = diag(U * V) for both nodes; A0 / A1: the nodes' tables
	// (`same`: one table, the shared-difference form).
	auto pair_rows = [&](auto PC, const PairWin& w, double (&rr)[2][9], const IsoAxis& A0, const IsoAxis& A1,
	                     bool same) {
		constexpr int P = decltype(PC)::value;
		if (KF0 && !same) {  // HET, two materials in the lane: per node, no shared differences
#pragma unroll
			for (int t = 0; t < 2; t++)
				pair_update<0, BS, true, P>(
				    t ? A1 : A0, [&](int j, int o) { return j == pair_vel(0, P) ? w[0][t + BS + o] : w[1][t + BS + o]; },
				    rr[t][2 * P], rr[t][2 * P + 1]);
		} else if constexpr (KF0 && !GCMX_FMA) {
			const IsoAxis& AS = A0;  // one table for both nodes
			const double* c = (P == 0) ? AS.c1 : AS.c2;
			double im[2][2], ip[2][2];  // [vel/sig][node]
#pragma unroll
			for (int v = 0; v < 2; v++) {
				double D[BS + 1][WX];
#pragma unroll
				for (int k = 0; k < WX; k++) D[0][k] = w[v][k];
#pragma unroll
				for (int i = 1; i <= BS; i++)
#pragma unroll
					for (int k = 0; k + i < WX; k++) D[i][k] = (D[i - 1][k + 1] - D[i - 1][k]) * c[i - 1];
#pragma unroll
				for (int t = 0; t < 2; t++) {
					const int m = t + BS;
					double a = D[0][m], b = D[0][m];
#pragma unroll
					for (int i = 1; i <= BS; i++) {
						a += D[i][m];
						b = (i % 2) ? b - D[i][m - i] : b + D[i][m - i];
					}
					// limiter segments (m, m+1) and (m, m-1): the median form (common.hpp
					// vlimit) takes three ops per foot, less than sharing the segment
					// bounds of node 0's +x foot with node 1's -x foot (2 + 2 per foot)
					ip[v][t] = vlimit(a, D[0][m], D[0][m + 1]);
					im[v][t] = vlimit(b, D[0][m], D[0][m - 1]);
				}
			}
#pragma unroll
			for (int t = 0; t < 2; t++) {
				rr[t][2 * P] = RowSum<0, false, 2 * P>::go(
				    AS, [&](int j) { return j == pair_vel(0, P) ? im[0][t] : im[1][t]; }, 0.0, true);
				rr[t][2 * P + 1] = RowSum<0, false, 2 * P + 1>::go(
				    AS, [&](int j) { return j == pair_vel(0, P) ? ip[0][t] : ip[1][t]; }, 0.0, true);
			}
		} else {
#pragma unroll
			for (int t = 0; t < 2; t++)
				pair_update<0, BS, KF0, P>(
				    t ? A1 : A0, [&](int j, int o) { return j == pair_vel(0, P) ? w[0][t + BS + o] : w[1][t + BS + o]; },
				    rr[t][2 * P], rr[t][2 * P + 1]);
		}
	};
	auto sched_fence = [] { __builtin_amdgcn_sched_barrier(0); };
	using P0 = std::integral_constant<int, 0>;
	using P1 = std::integral_constant<int, 1>;
	using P2 = std::integral_constant<int, 2>;
	// X-stage inputs issued ahead of the X stage: load pairs 0 and 1.
	struct XPre {
		PairWin a, b;
	};
	auto cv_load = [&](double (&cv)[2][9], int r) {
		if constexpr (WIDE) {  // the own planes as one pair (raw: half_swap in x_compute)
#pragma unroll
			for (int j = 0; j < 9; j++)
				if ((CMX >> j) & 1u) {
					const dpair v = ldw(j, BS, BS + 1, r, true);
					cv[0][j] = v.x, cv[1][j] = v.y;
				}
			return;
		}
#pragma unroll
		for (int t = 0; t < 2; t++)
#pragma unroll
			for (int j = 0; j < 9; j++)
				if ((CMX >> j) & 1u) cv[t][j] = ldc(j, BS + t, r);
	};
	auto x_load_ahead = [&](XPre& pre, int r) {
		pair_load(P0{}, pre.a, r);
		pair_load(P1{}, pre.b, r);
	};
	// X stage of row r for both nodes: pair 2 and the node-only components are
	// issued first, then the pairs are consumed in order.
	// material of node (x + t, r) (HET; rows outside [0, Y) take row Y-1's: their
	// X results come from zero ghost rows or are replaced by a face's mirror)
	auto mat_of = [&](int t, int r) -> unsigned {
		const int xx = (t == 1 && !two) ? x : (t == 0 && !one) ? x + 1 : x + t;
		const int rr_ = r < 0 ? 0 : (r < Y ? r : Y - 1);
		return mat[((size_t)xx * Y + rr_) * Z + z];
	};
	auto x_compute = [&](const XPre& pre, const PairWin& wc_, const double (&cv_)[2][9], double (&xr)[2][9],
	                     const IsoAxis& A0, const IsoAxis& A1, bool same) {
		double rr[2][9], n0[2][9], cv[2][9];
		PairWin pa, pb, wc;
		pair_fix(pre.a, pa);
		pair_rows(P0{}, pa, rr, A0, A1, same);
		pair_fix(pre.b, pb);
		pair_rows(P1{}, pb, rr, A0, A1, same);
		sched_fence();
		pair_fix(wc_, wc);
		pair_rows(P2{}, wc, rr, A0, A1, same);
#pragma unroll
		for (int t = 0; t < 2; t++) {
			n0[t][pair_vel(0, 0)] = pa[0][t + BS];
			n0[t][pair_sig(0, 0)] = pa[1][t + BS];
			n0[t][pair_vel(0, 1)] = pb[0][t + BS];
			n0[t][pair_sig(0, 1)] = pb[1][t + BS];
			n0[t][pair_vel(0, 2)] = wc[0][t + BS];
			n0[t][pair_sig(0, 2)] = wc[1][t + BS];
		}
		sched_fence();
#pragma unroll
		for (int j = 0; j < 9; j++)
			if ((CMX >> j) & 1u) {
				cv[0][j] = cv_[0][j], cv[1][j] = cv_[1][j];
				if constexpr (WIDE) half_swap(cv[0][j], cv[1][j]);
			}
#pragma unroll
		for (int t = 0; t < 2; t++) {
			const IsoAxis& A = t ? A1 : A0;
			center_update<0>(A, [&](int j) { return ((WMX >> j) & 1u) ? n0[t][j] : cv[t][j]; }, rr[t]);
			u1_apply<0>(A, rr[t], xr[t]);
		}
	};
	// HET: the two nodes' materials of row r as one key (node x in bits 0-7)
	auto key_of = [&](int r) -> unsigned { return mat_of(0, r) | (mat_of(1, r) << 8); };
	// key: key_of(r), loaded ahead by the caller (HET)
	auto x_stage = [&](const XPre& pre, int r, double (&xr)[2][9], unsigned key) {
		PairWin wc;
		double cv[2][9];
		pair_load(P2{}, wc, r);
		cv_load(cv, r);
		sched_fence();
		if constexpr (HET) {
			const unsigned m0 = key & 255u, m1 = key >> 8;
			x_compute(pre, wc, cv, xr, mt(m0), mt(m1), m0 == m1);
		} else {
			x_compute(pre, wc, cv, xr, AX, AX, true);
		}
	};

	double win[2][NWY][W];
	// HET: material keys of the window's rows (slot k: row y - BS + k), each loaded
	// once, one row ahead of its X stage, and reused by that row's Y and Z stages
	unsigned hk[W];
#pragma unroll
	for (int k = 0; k < W; k++) hk[k] = 0;
	if constexpr (HET) {  // tables into LDS (het tables are allocated for 256 materials)
		for (int i = z; i < kHetMaxMaterials * (int)(sizeof(IsoAxis) / 4); i += ZT)
			reinterpret_cast<unsigned*>(hlds)[i] = reinterpret_cast<const unsigned*>(mtab)[i];
		if (fb.ode_on && fb.ode_f && z < kHetMaxMaterials) hode[z] = fb.ode_f[z];
	}
	if constexpr (HET) __syncthreads();
	// The row march, in either direction (REV: from the chunk's last row down).
	// Odd chunks march down, so the halo rows two adjacent chunks both compute
	// the X stage of are read by both blocks at the same time -- both at the
	// start or both at the end of their march -- and the second read hits the
	// caches (a forward-only march reads them at opposite ends of the launch:
	// 256^3, 64-row chunks, 1.13x the compulsory reads from HBM).
	auto run = [&](auto RV) {
	constexpr bool REV = decltype(RV)::value;
	constexpr int S = REV ? -1 : 1;
	// node-only Y components: ring slot of row r; per-lane pointer with the
	// (node, component) part as a constant LDS offset
	auto cl_at = [&](int r) { return &cl[(r + 2 * BS + 2) % (BS + 1)][0][0][ci]; };
	// row r's X result enters window slot `slot`; its node-only components go to the ring
	auto push = [&](const double (&xr)[2][9], int slot, int r) {
		double* cp = cl_at(r);
#pragma unroll
		for (int t = 0; t < 2; t++)
#pragma unroll
			for (int j = 0; j < 9; j++) {
				if ((WMY >> j) & 1u) win[t][wslot(WMY, j)][slot] = xr[t][j];
				if ((CMY >> j) & 1u) cp[(t * NCY + wslot(CMY, j)) * ZT] = xr[t][j];
			}
	};
	// window slot k := ghost of face f mirrored from window slot ks (a runtime
	// index, resolved by compile-time selects; rare path)
	auto mirror_slot = [&](int k, int ks, int f) {
#pragma unroll
		for (int t = 0; t < 2; t++) {
			const GhostRule gr = ghost_rule(f, t, zg, WMY);
#pragma unroll
			for (int q = 0; q < NWY; q++) {
				double v = 0.0;
#pragma unroll
				for (int kk = 0; kk < W; kk++)
					if (kk == ks) v = win[t][q][kk];
				const double gv = ghost(gr, wcomp(WMY, q), v);
#pragma unroll
				for (int kk = 0; kk < W; kk++)
					if (kk == k) win[t][q][kk] = gv;
			}
		}
	};
	// prologue: X results of rows y0-BS .. y0+BS (rows < 0 or >= Y are ghosts);
	// window slot k holds row y + S*(k - BS) of the current row y
	const int y0 = REV ? ye - 1 : yb;
#pragma unroll
	for (int k = 0; k < W; k++) {
		const int r = y0 + S * (k - BS);
		double xr[2][9];
		if (r >= 0 && r < Y) {
			XPre pre;
			if constexpr (HET) hk[k] = key_of(r);
			x_load_ahead(pre, r);
			x_stage(pre, r, xr, hk[k]);
		} else {
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int j = 0; j < 9; j++) xr[t][j] = 0.0;
		}
		push(xr, k, r);  // the first BS rows are overwritten in the ring by the last BS
	}
	if constexpr (FACES) {  // ghost rows of the prologue window: mirrors of inner rows
		if (fb.on & 3u) {
#pragma unroll
			for (int k = 0; k < W; k++) {
				const int r = y0 + S * (k - BS);
				const int f = r < 0 ? 0 : 1, ks = BS + S * ((r < 0 ? -r : 2 * (Y - 1) - r) - y0);
				if ((r < 0 || r >= Y) && ((fb.on >> f) & 1u) && ks >= 0 && ks < W) mirror_slot(k, ks, f);
			}
		}
	}
	auto clamp_row = [&](int r) {  // rows beyond the ghost rows (their X results go unused)
		if constexpr (REV) return r > -BS ? r : -BS;
		return r < Y + BS - 1 ? r : Y + BS - 1;
	};

	// Y stage of row y for both nodes (window + node-only ring)
	auto y_stage = [&](int y, double (&yv)[2][9]) {
		const double* cp = cl_at(y);
#pragma unroll
		for (int t = 0; t < 2; t++) {
			auto go = [&](const IsoAxis& A) {
				node_update<1, BS, KF0>(
				    A, [&](int j, int o) { return win[t][wslot(WMY, j)][BS + S * o]; },
				    [&](int j) { return ((WMY >> j) & 1u) ? win[t][wslot(WMY, j)][BS] : cp[(t * NCY + wslot(CMY, j)) * ZT]; },
				    yv[t]);
			};
			if constexpr (HET) go(mt(t ? hk[BS] >> 8 : hk[BS] & 255u));
			else go(AY);
		}
	};
	// z ghosts of row y (FACES): lanes 1..BS form the z- face's ghost columns,
	// lanes Z-1-BS..Z-2 the z+ face's, put(side, node, window slot, value) -- one
	// divergent region per face and row, entered only by the waves holding those
	// lanes, one condition lookup per node
	auto z_ghosts = [&](int y, const double (&yv)[2][9], auto&& put) {
		const int wu = __builtin_amdgcn_readfirstlane(z >> 6);
#pragma unroll
		for (int side = 0; side < 2; side++) {
			// ZS: the z- face lies in the first part, the z+ face in the last, at
			// lanes of that part (Zl: the part's row length)
			const int Zl = ZS ? ZT : Z;
			if (ZS && (side ? zp != nz - 1 : zp != 0)) continue;
			const int lo = side ? Zl - 1 - BS : 1, hi = side ? Zl - 2 : BS;
			if (!((fb.on >> (2 + side)) & 1u) || wu * 64 > hi || wu * 64 + 63 < lo) continue;
			if (z < lo || z > hi) continue;
#pragma unroll
			for (int t = 0; t < 2; t++) {
				const GhostRule gr = ghost_rule(2 + side, t, y, WMZ);
#pragma unroll
				for (int j = 0; j < 9; j++)
					if ((WMZ >> j) & 1u) put(side, t, wslot(WMZ, j), ghost(gr, j, yv[t][j]));
			}
		}
	};
	// hand the Y results of row y to the Z stage: NB, own region + edge ring +
	// counter; otherwise the block buffer between two barriers
	auto publish = [&](int it, int y, const double (&yv)[2][9]) {
		const int es = it & 1;  // NB: edge ring slot of this row (it: the row's place in the march)
		if constexpr (NB) {
			// this lane's edge slot (lanes < BS: left side, >= 64 - BS: right side);
			// (node, component) as a constant LDS offset
			double* egp = ln < BS ? &eg[es][wv][0][0][0][ln] : &eg[es][wv][1][0][0][ln - (64 - BS)];
			const bool edge = ln < BS || ln >= 64 - BS;
			asm volatile("" ::: "memory");  // after the previous row's Z-stage reads of rg
			// The edges first: the neighbour waves wait for them, while the own region
			// (and the face ghosts) is read by this wave's own Z stage only, whose LDS
			// reads come after these writes anyway.
			if (edge) {
#pragma unroll
				for (int t = 0; t < 2; t++)
#pragma unroll
					for (int j = 0; j < 9; j++)
						if ((WMZ >> j) & 1u) egp[(t * NWZ + wslot(WMZ, j)) * BS] = yv[t][j];
			}
			// edges in LDS before the counter says so (LDS only: global memory keeps flowing)
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__hip_atomic_store(&rdy[wv], it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			asm volatile("" ::: "memory");
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int j = 0; j < 9; j++)
					if ((WMZ >> j) & 1u) rg[wv][t][wslot(WMZ, j)][rs0] = yv[t][j];
			if constexpr (FACES)  // z ghosts: wave 0's left halo, the last wave's right halo
				z_ghosts(y, yv, [&](int side, int t, int q, double v) {
					if (side == 0) rg[0][t][q][rs(-z)] = v;
					else rg[NW - 1][t][q][rs(2 * ((ZS ? ZT : Z) - 1) - z - 64 * (NW - 1))] = v;
				});
		} else {
			__syncthreads();  // every wave has finished reading zl (previous row's Z stage)
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int j = 0; j < 9; j++)
					if ((WMZ >> j) & 1u) {
						const int q = wslot(WMZ, j);
						if constexpr (FACES) {
							// idle lanes leave the z ghost slots to the face (or their zero)
							if (UNI || z < Z || z >= Z + BS) zl[t][q][BS + z] = live ? yv[t][j] : 0.0;
						} else {
							zl[t][q][BS + z] = live ? yv[t][j] : 0.0;
						}
					}
			if constexpr (FACES)
				z_ghosts(y, yv, [&](int side, int t, int q, double v) {
					if (side == 0) zl[t][q][BS - z] = v;
					else zl[t][q][BS + 2 * (Z - 1) - z] = v;
				});
			__syncthreads();
		}
	};
	// NB: wait for the neighbour waves' edges of row y, copy them into the own halo slots
	auto collect = [&](int it) {
		if constexpr (NB && NW > 1) {
			const int es = it & 1;
			for (;;) {
				const int a = wv > 0 ? __hip_atomic_load(&rdy[wv - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : it;
				const int b =
				    wv < NW - 1 ? __hip_atomic_load(&rdy[wv + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : it;
				if (__builtin_amdgcn_readfirstlane(min(a, b)) >= it) break;
				__builtin_amdgcn_s_sleep(1);  // a neighbour wave's edges are not there yet
			}
			asm volatile("" ::: "memory");
			// One edge value per hand-over lane, both sides in one LDS read and one
			// write (hpk above, unpacked here each row).  Ordering: the flags and the ring are as they
			// were -- a neighbour's edges of row `it` are in `eg` before its counter
			// says so, and it overwrites this ring row only at row it + 2, after its
			// collect of row it + 1 has seen this wave's counter at it + 1, which this
			// wave sets after the read below has returned (publish's lgkmcnt(0)).
			// Which lanes copy does not matter to the Z stage: the same wave does
			// the copy and the Z-stage reads of its halo, and a wave's LDS operations
			// complete in order.
			const unsigned p = opaque_u32(hpk);
			if ((int)p >= 0) (&rg[0][0][0][0])[p >> 16] = (&eg[0][0][0][0][0][0])[(p & 0xFFFFu) + (unsigned)(es * ESZ)];
			asm volatile("" ::: "memory");
		}
	};
	// Z stage of node t of row y and its 9 stores (WIDE: the results to zv, stored
	// by z_store_wide once both nodes' are there)
	auto z_stage_store = [&](int t, int y, const double (&yv)[2][9], double (&zv)[9]) {
		auto go = [&](const IsoAxis& A) {
			if constexpr (NB)
				node_update<2, BS, KF0>(
				    A, [&](int j, int o) { return rg[wv][t][wslot(WMZ, j)][rso(o)]; },
				    [&](int j) { return ((WMZ >> j) & 1u) ? rg[wv][t][wslot(WMZ, j)][rs0] : yv[t][j]; }, zv);
			else
				node_update<2, BS, KF0>(
				    A, [&](int j, int o) { return zl[t][wslot(WMZ, j)][BS + z + o]; },
				    [&](int j) { return ((WMZ >> j) & 1u) ? zl[t][wslot(WMZ, j)][BS + z] : yv[t][j]; }, zv);
		};
		if constexpr (HET) go(mt(t ? hk[BS] >> 8 : hk[BS] & 255u));
		else go(AZ);
		if (fb.ode_on) {  // MaxwellViscosityOde: sigma *= exp(-tau / tau0), the stored product (Ode.hpp:34-35)
			double f = fb.ode;
			if constexpr (HET)  // the node's own material's factor
				if (fb.ode_f) f = hode[t ? hk[BS] >> 8 : hk[BS] & 255u];
#pragma unroll
			for (int c = 3; c < 9; c++) zv[c] = zv[c] * f;
		}
		if constexpr (WIDE) return;
		if ((t == 0 ? one : two) && !(ZS && seam_own)) {
#pragma unroll
			for (int c = 0; c < 9; c++) stz(c, t, y, live ? zv[c] : 0.0);
		}
	};
	// WIDE: both nodes' results of row y, 9 16-byte stores: plane x from the lower
	// half-wave, plane x + 1 from the upper
	auto z_store_wide = [&](int y, double (&zv)[2][9]) {
#pragma unroll
		for (int c = 0; c < 9; c++) half_swap(zv[0][c], zv[1][c]);
		if ((hsel ? two : one) && !seam_pair) {
#pragma unroll
			for (int c = 0; c < 9; c++) stw(c, y, zv[0][c], zv[1][c]);
		}
	};
	// X stage of row y+S*(BS+1) -> window slot W-1 (ghost rows: zero, or a face's mirror)
	auto x_enter = [&](int y, const XPre& pre, unsigned kn) {
#pragma unroll
		for (int t = 0; t < 2; t++)
#pragma unroll
			for (int q = 0; q < NWY; q++)
#pragma unroll
				for (int o = 0; o < W - 1; o++) win[t][q][o] = win[t][q][o + 1];
		if constexpr (HET) {
#pragma unroll
			for (int o = 0; o < W - 1; o++) hk[o] = hk[o + 1];
			hk[W - 1] = kn;
		}
		double xr[2][9];
		sched_fence();
		const int r = y + S * (BS + 1);
		x_stage(pre, clamp_row(r), xr, kn);
		push(xr, W - 1, r);
		sched_fence();
		if constexpr (FACES) {
			const int f = r < 0 ? 0 : 1;
			if ((r < 0 || r >= Y) && ((fb.on >> f) & 1u)) {  // slot of the mirrored row in the next row's window
				const int ks = BS + S * ((r < 0 ? -r : 2 * (Y - 1) - r) - (y + S));
				if (ks >= 0 && ks < W) mirror_slot(W - 1, ks, f);
			}
		}
	};
	auto row = [&](int y, int it) {
		double yv[2][9], zv[2][9];
		XPre pre;
		const int rn = clamp_row(y + S * (BS + 1));
		unsigned kn = 0;  // HET: row rn's materials, one row ahead of its X stage
		if constexpr (HET) kn = key_of(rn);
		y_stage(y, yv);
		publish(it, y, yv);
		if constexpr (ZS2) {
			sched_fence();
			pair_load(P0{}, pre.a, rn);
			sched_fence();
		} else {  // loads older than this row's stores
			sched_fence();
			x_load_ahead(pre, rn);
			sched_fence();
		}
		collect(it);
#pragma unroll
		for (int t = 0; t < 2; t++) {  // each node's stores right after its Z stage
			if constexpr (ZS2) {
				if (t == 1) {
					sched_fence();
					pair_load(P1{}, pre.b, rn);
					sched_fence();
				}
			}
			z_stage_store(t, y, yv, zv[t]);
		}
		if constexpr (WIDE) z_store_wide(y, zv);
		x_enter(y, pre, kn);
	};
	for (int it = 0; it < ye - yb; it++) row(REV ? ye - 1 - it : yb + it, it);
#if GCMX_TX2_BLKT
	if ((threadIdx.x & 63) == 0 && blockIdx.x < (unsigned)kBlkMax && threadIdx.x < 512) {
		const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
		g_tx2_blk[blockIdx.x][threadIdx.x / 64][0] = blk_t0_;
		g_tx2_blk[blockIdx.x][threadIdx.x / 64][1] = t1;
		if (threadIdx.x == 0) g_tx2_hw[blockIdx.x] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_HW_ID
	}
#endif
	};
	if (rev) run(std::true_type{});
	else run(std::false_type{});
}

// The nodes next to the cuts of a z-split step (k_step_tx2<..., ZS>), after it:
// lane (plane, column) of a group of 4*BS lanes holds one of the columns
// cut - 2*BS ... cut + 2*BS - 1 of one x plane and marches y like k_fused_xyz --
// the X stage of the entering row (node_update<0>: the same per-node operations
// as the one-pass step's X stage), the Y stage from its register window -- then
// the Z stage of the middle 2*BS columns from the group's Y results (lane
// shuffles), the folded ODE factor, 9 stores.  Rows: `chunk` per block, the
// 2*BS-row prologue recomputed.  Reads the 4*BS columns' neighbourhoods (mostly
// L2), writes 2*BS columns per cut: at 1024^3 0.4 % of the step's bytes.
//
// FACES: y-face conditions as the one-pass step forms them (FaceBC, uniform or a
// per-node map): a window row outside [0, Y) is the mirrored inner row with the
// condition's components set to -inner + 2 f(t) (BorderConditions.hpp:94-114).
template <int BS, bool KF0, bool FACES>
__global__ __launch_bounds__(256) void k_zseam(const double* __restrict__ in, double* __restrict__ outl, Geo g,
                                                IsoAxis A, int x0, int nplanes, int xb0, int nplanesb, int zt,
                                                int chunk, FaceBC fb) {
	const unsigned ode_on = fb.ode_on;
	const double ode = fb.ode;
	constexpr int NC = 4 * BS, PB = 256 / NC, W = 2 * BS + 1;
	const int Y = g.sizes[1], ncut = g.sizes[2] / zt - 1;
	const int nch = (Y + chunk - 1) / chunk;
	int b = (int)blockIdx.x;
	const int ch = b % nch;
	b /= nch;
	const int cut = b % ncut;
	const int pg = b / ncut;
	const int c = (int)threadIdx.x % NC, xi = pg * PB + (int)threadIdx.x / NC;
	const bool valid = xi < nplanes + nplanesb;
	const int x = !valid ? x0 : xi < nplanes ? x0 + xi : xb0 + (xi - nplanes);
	const int z = (cut + 1) * zt - 2 * BS + c;
	const long long stx = g.stride[0], sty = g.stride[1], cs = g.cs;
	const long long base = g.origin + (long long)x * stx + z;
	const int yb = ch * chunk, ye = min(yb + chunk, Y);
	// X result of row r (rows outside [0, Y): zero ghost rows; beyond them clamped)
	auto xstage = [&](int r, double (&xr)[9]) {
		const int rc = r < -BS ? -BS : (r > Y + BS - 1 ? Y + BS - 1 : r);
		const long long o = base + (long long)rc * sty;
		node_update<0, BS, KF0>(
		    A, [&](int j, int oo) { return in[j * cs + o + oo * stx]; }, [&](int j) { return in[j * cs + o]; }, xr);
	};
	double win[9][W];
	// window slot k := the ghost of y face f mirrored from slot ks (runtime slot
	// indices resolved by compile-time selects, as k_step_tx2's mirror_slot)
	auto mirror = [&](int k, int ks, int f) {
		unsigned mask;
		bool none = false;
		double two[9];
		if (fb.map[f]) {
			const unsigned cnd = fb.map[f][(size_t)x * g.sizes[2] + z];
			none = cnd == kNoFaceCond;
			const FaceCond& fc = fb.conds[none ? 0u : cnd];
			mask = none ? 0u : fc.mask;
#pragma unroll
			for (int j = 0; j < 9; j++) two[j] = none ? 0.0 : fc.two_v[j];
		} else {
			mask = fb.mask[f];
#pragma unroll
			for (int j = 0; j < 9; j++) two[j] = fb.two_v[f][j];
		}
#pragma unroll
		for (int j = 0; j < 9; j++) {
			double v = 0.0;
#pragma unroll
			for (int kk = 0; kk < W; kk++)
				if (kk == ks) v = win[j][kk];
			const double gv = none ? 0.0 : ((mask >> j) & 1u) ? -v + two[j] : v;
#pragma unroll
			for (int kk = 0; kk < W; kk++)
				if (kk == k) win[j][kk] = gv;
		}
	};
#pragma unroll
	for (int k = 0; k < W; k++) {
		double xr[9];
		const int r = yb - BS + k;
		if (r >= 0 && r < Y) xstage(r, xr);
		else
#pragma unroll
			for (int j = 0; j < 9; j++) xr[j] = 0.0;
#pragma unroll
		for (int j = 0; j < 9; j++) win[j][k] = xr[j];
	}
	if constexpr (FACES) {  // ghost rows of the prologue window: mirrors of inner rows
		if (fb.on & 3u) {
#pragma unroll
			for (int k = 0; k < W; k++) {
				const int r = yb - BS + k;
				const int f = r < 0 ? 0 : 1, ks = BS + ((r < 0 ? -r : 2 * (Y - 1) - r) - yb);
				if ((r < 0 || r >= Y) && ((fb.on >> f) & 1u) && ks >= 0 && ks < W) mirror(k, ks, f);
			}
		}
	}
	const bool mine = valid && c >= BS && c < 3 * BS;  // the columns whose Z stage the parts left
	const int lane = (int)(threadIdx.x & 63);
	for (int y = yb; y < ye; y++) {
		double yv[9], zv[9];
		node_update<1, BS, KF0>(A, [&](int j, int o) { return win[j][BS + o]; }, [&](int j) { return win[j][BS]; }, yv);
		// z neighbours: lanes c +- o of the same group (the group never straddles a wave)
		node_update<2, BS, KF0>(
		    A, [&](int j, int o) { return __shfl(yv[j], lane + o, 64); }, [&](int j) { return yv[j]; }, zv);
		if (mine) {
			if (ode_on) {
#pragma unroll
				for (int k = 3; k < 9; k++) zv[k] = zv[k] * ode;
			}
			const long long off = base + (long long)y * sty;
#pragma unroll
			for (int k = 0; k < 9; k++) __builtin_nontemporal_store(zv[k], outl + k * cs + off);
		}
#pragma unroll
		for (int j = 0; j < 9; j++)
#pragma unroll
			for (int k = 0; k < W - 1; k++) win[j][k] = win[j][k + 1];
		double xr[9];
		const int r = y + BS + 1;
		if (r < Y) xstage(r, xr);
		else
#pragma unroll
			for (int j = 0; j < 9; j++) xr[j] = 0.0;
#pragma unroll
		for (int j = 0; j < 9; j++) win[j][W - 1] = xr[j];
		if constexpr (FACES) {  // the entering row is a y+ ghost row: the mirror of an inner row
			if (r >= Y && ((fb.on >> 1) & 1u)) {
				const int ks = BS + (2 * (Y - 1) - r) - (y + 1);
				if (ks >= 0 && ks < W) mirror(W - 1, ks, 1);
			}
		}
	}
}

// ------------------------------------------------------------- launchers --

static bool same_axis(const IsoAxis& p, const IsoAxis& q) {  // bitwise
	static_assert(sizeof(IsoAxis) == 18 * 8 + 2 * 4, "IsoAxis has padding");
	return std::memcmp(&p, &q, sizeof(IsoAxis)) == 0;
}

// The instance a launch runs, as a readable symbol (gcmx_profile_kernel).
// Which access path ran: a UNI instance takes the 16-byte path and keeps its
// plain name (the one the committed PMC records carry); ", N8" marks a UNI
// launch that fell back to 8-byte accesses (odd strides, or an instance kept
// narrow).  The !UNI instances have the 8-byte path only.
template <int BS, int ZT, bool KF0, bool UNI, bool FACES, bool HET, bool ZS = false, bool WD = false>
static const char* tx2_name() {
	static const std::string s = "k_step_tx2<" + std::to_string(BS) + ", " + std::to_string(ZT) + ", " +
	                             (KF0 ? "KF0" : "!KF0") + ", " + (UNI ? "UNI" : "!UNI") + ", " +
	                             (FACES ? "FACES" : "!FACES") + (HET ? ", HET" : "") + (ZS ? ", ZS" : "") +
	                             (UNI && !WD ? ", N8" : "") + GCMX_FP_TAG + ">";
	return s.c_str();
}
// The barrier-free instances (UNI) take the wide path when the launch allows it.
static bool tx2_wide_ok(const Geo& g, const double* in, const double* out) {
	return wide_layout_ok(g) && (((uintptr_t)in | (uintptr_t)out) & 15u) == 0;
}
template <int BS, int ZT, bool KF0, bool UNI>
static const char* xyz_name() {
	static const std::string s = "k_fused_xyz<" + std::to_string(BS) + ", " + std::to_string(ZT) + ", " +
	                             (KF0 ? "KF0" : "!KF0") + ", " + (UNI ? "UNI" : "!UNI") + GCMX_FP_TAG + ">";
	return s.c_str();
}

// Rows per block of k_step_tx2 (req > 0 forces a value): the longest chunk of
// the form Y, 512, 256, ..., 16 whose launch still fills >= 90 % of the resident
// block slots (`slots` = CUs x blocks per CU), so one round of blocks covers the
// launch with the fewest 2*BS-row prologues (measured, DESIGN.md §3.1 / §5:
// 512^3 512 rows 4.32 vs 256 rows 4.37 ms; a 60-plane slab interior 64 rows
// 0.54 vs 32 rows 0.56 vs 16 rows 0.60 ms; 256^3 64 rows 0.590 vs 32 / 128 rows
// 0.599 / 0.692 ms).
static int tx2_chunk_for(int Y, int npair, int req, int slots) {
	if (req > 0) return Y <= req ? Y : req;
	for (int t = 1024; t >= 16; t /= 2) {
		const int ch = Y < t ? Y : t;
		if (10LL * npair * ((Y + ch - 1) / ch) >= 9LL * slots) return ch;
	}
	return Y < 16 ? Y : 16;
}

static int device_cus();
// Two generations of rows (k_step_tx2's chunk < 0): when a launch is exactly two
// resident blocks per CU, the block dispatched first to a CU finishes ~25 %
// before its co-resident younger block (256^3: 0.40 against 0.51 ms,
// profiles/r6/r), and the CU runs the rest at half occupancy.  Old blocks then
// take `co` rows and young ones `cy` (co + cy = 2 Y / nchunk; GCMX_TX2_GEN2 =
// the old share in percent, 0 = off).  Returns the kernel's chunk argument.
static int tx2_gen2(int Y, int npair, int chunk, int T, int per_cu) {
	static const int pct = [] {
		const char* e = std::getenv("GCMX_TX2_GEN2");
		return e ? std::atoi(e) : kTx2Gen2Default;
	}();
	if (pct <= 50 || pct >= 100 || per_cu != 2 || T != 2 * device_cus() || T % 16 || (T / 2) % npair) return chunk;
	const int nchunk = T / npair;
	if (Y % chunk || Y / chunk != nchunk) return chunk;
	const int ncg = nchunk / 2, two = Y / ncg;  // rows of one old + one young chunk
	if (two * ncg != Y) return chunk;
	const int co = (two * pct + 50) / 100, cy = two - co;
	if (cy < 2 * 2 + 1 || co > 0xFFFF) return chunk;
	return -(co | (cy << 16));
}

static int device_cus() {
	static int n = [] {
		int dev = 0, v = 0;
		if (hipGetDevice(&dev) != hipSuccess ||
		    hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
			v = 256;
		return v;
	}();
	return n;
}

// z split (k_step_tx2<BS, P, ..., ZS> + k_zseam): parts of P lanes, uniform
// medium (equal axes, floor(q) = 0); FACES: the y/z face conditions.
template <int BS, int P, bool FACES>
static void launch_zs(const double* in, double* out, const Geo& g, const IsoAxis* a, int x0, int x1, int xb0, int xb1,
                      hipStream_t st, int req_chunk, const FaceBC* fb, const char** kname) {
	const int nz = g.sizes[2] / P, nb = xb1 > xb0 ? xb1 - xb0 : 0;
	const int npair = (x1 - x0 + ((g.gx0 + x0) & 1) + 1) / 2 + (nb > 0 ? (nb + ((g.gx0 + xb0) & 1) + 1) / 2 : 0);
	// 128 rows per block unless asked: 1024^3 35.2 ms against 36.3 (256 rows),
	// 36.6 (64) and 39.0 (1024, the one-round rule of the Z <= 512 step),
	// profiles/r6/e
	const int chunk = req_chunk > 0 ? std::min(req_chunk, g.sizes[1]) : std::min(128, g.sizes[1]);
	const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * npair * nz);
	const FaceBC none{};
	const FaceBC& f = fb ? *fb : none;
	auto go = [&](auto WDC) {
		constexpr bool WD = decltype(WDC)::value;
		hipLaunchKernelGGL((k_step_tx2<BS, P, true, true, FACES, false, true, WD>), grid, dim3(P), 0, st, in, out, g,
		                   a[0], a[1], a[2], x0, chunk, x1 - x0, xb0, nb, f, nullptr, nullptr);
		*kname = tx2_name<BS, P, true, true, FACES, false, true, WD>();
	};
	if (tx2_wide_ok(g, in, out)) go(std::true_type{});
	else go(std::false_type{});
	// the cut columns: 256 / (4 BS) planes per block, 64-row chunks
	const int np = (x1 - x0) + nb, pb = 256 / (4 * BS), sch = std::min(64, g.sizes[1]);
	const long long nblk = (long long)((np + pb - 1) / pb) * (nz - 1) * ((g.sizes[1] + sch - 1) / sch);
	hipLaunchKernelGGL((k_zseam<BS, true, FACES>), dim3((unsigned)nblk), dim3(256), 0, st, in, out, g, a[0], x0,
	                   x1 - x0, xb0, nb, P, sch, f);
}

template <int BS, int ZT>
static void launch_xyz_t(const double* in, double* out, const Geo& g, const IsoAxis* a, int x0,
                         int x1, int xb0, int xb1, hipStream_t st, int req_chunk, const FaceBC* fb,
                         const char** kname, const HetMaterials* het) {
	bool kf0 = true;
	for (int s = 0; s < 3; s++) kf0 = kf0 && a[s].kf1 == 0 && a[s].kf2 == 0;
	const bool uni = kf0 && g.sizes[2] == ZT && same_axis(a[0], a[1]) && same_axis(a[0], a[2]);
	if constexpr (BS <= 2 && ZT <= 512) {
		const int nb = xb1 > xb0 ? xb1 - xb0 : 0;
		// global pairs (k_step_tx2): a range starting at an odd global plane
		// begins with a half pair
		const int npair = (x1 - x0 + ((g.gx0 + x0) & 1) + 1) / 2 +
		                  (nb > 0 ? (nb + ((g.gx0 + xb0) & 1) + 1) / 2 : 0);
		// resident blocks: 2 waves per SIMD (<= 256 VGPRs), i.e. 512 / ZT per CU
		const int chunk = tx2_chunk_for(g.sizes[1], npair, req_chunk, device_cus() * (512 / ZT));
		const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * npair);
		const int cparam = req_chunk > 0 ? chunk : tx2_gen2(g.sizes[1], npair, chunk, (int)grid.x, 512 / ZT);
		const FaceBC none{};
		const FaceBC& f = fb ? *fb : none;
		const IsoAxis* mt = het ? het->tab : nullptr;
		const uint8_t* mi = het ? het->ids : nullptr;
		auto go = [&](auto K, const char* name) {
			hipLaunchKernelGGL(K, grid, dim3(ZT), 0, st, in, out, g, a[0], a[1], a[2], x0, cparam, x1 - x0, xb0,
			                   nb, f, mt, mi);
			*kname = name;
		};
		// the UNI instances: 16-byte accesses where the layout allows, else the 8-byte path
		const bool wide = tx2_wide_ok(g, in, out);
		auto go_uni = [&](auto FC, auto HC) {
			constexpr bool F = decltype(FC)::value, H = decltype(HC)::value;
			// per-node materials at borderSize 2 keep the 8-byte path: holding node
			// 0's results across node 1's Z stage spills there (24-80 B of scratch)
			// and so do the 256-lane instances: with two blocks per CU the wide path
			// measured slower (256^3: 4 of 5 alternating pairs, +0.5 .. +4.6 %,
			// profiles/wide/bench_256_*.jsonl), against -2.3 % at one 512-lane block
			constexpr bool W = !(H && BS == 2) && ZT != 256;
			if (wide && W) go(k_step_tx2<BS, ZT, true, true, F, H, false, W>,
			                  tx2_name<BS, ZT, true, true, F, H, false, W>());
			else go(k_step_tx2<BS, ZT, true, true, F, H>, tx2_name<BS, ZT, true, true, F, H>());
		};
		if (het) {  // the caller checked Z == ZT, KF0 and equal axes per material
			if (fb && fb->on) go_uni(std::true_type{}, std::true_type{});
			else go_uni(std::false_type{}, std::true_type{});
			return;
		}
		if (fb && fb->on) {
			if (uni) go_uni(std::true_type{}, std::false_type{});
			else if (kf0) go(k_step_tx2<BS, ZT, true, false, true, false>, tx2_name<BS, ZT, true, false, true, false>());
			else go(k_step_tx2<BS, ZT, false, false, true, false>, tx2_name<BS, ZT, false, false, true, false>());
		} else {
			if (uni) go_uni(std::false_type{}, std::false_type{});
			else if (kf0) go(k_step_tx2<BS, ZT, true, false, false, false>, tx2_name<BS, ZT, true, false, false, false>());
			else go(k_step_tx2<BS, ZT, false, false, false, false>, tx2_name<BS, ZT, false, false, false, false>());
		}
		return;
	}
	// borderSize 3, or a row longer than 512.  (The rest of this function is not
	// reached at borderSize <= 2, ZT <= 512, but stays outside an `else`: that
	// would drop those k_fused_xyz instances from the code object.)
	if (xb1 > xb0) {  // k_fused_xyz has no second range: two launches
		launch_xyz_t<BS, ZT>(in, out, g, a, x0, x1, 0, 0, st, req_chunk, fb, kname, het);
		x0 = xb0;
		x1 = xb1;
	}
	const int chunk = plane_chunk_for(g.sizes[1], x1 - x0, req_chunk);
	const dim3 grid(((g.sizes[1] + chunk - 1) / chunk) * (x1 - x0));
	auto go1 = [&](auto KC, auto UC) {
		constexpr bool K = decltype(KC)::value, U = decltype(UC)::value;
		hipLaunchKernelGGL((k_step_plane<IsoAxis, BS, ZT, K, U, false>), grid, dim3(ZT), 0, st, in, out, g, a[0], a[1],
		                   a[2], x0, chunk, x1 - x0, PlaneHet<IsoAxis>{});
		*kname = xyz_name<BS, ZT, K, U>();
	};
	if (uni) go1(std::true_type{}, std::true_type{});
	else if (kf0) go1(std::true_type{}, std::false_type{});
	else go1(std::false_type{}, std::false_type{});
}

template <int BS>
static bool launch_xyz_bs(const double* in, double* out, const Geo& g, const IsoAxis* a, int x0,
                          int x1, int xb0, int xb1, hipStream_t st, int ch, const FaceBC* fb,
                          const char** kn, const HetMaterials* het) {
	with_row_lanes(g.sizes[2], [&](auto ZC) {
		launch_xyz_t<BS, decltype(ZC)::value>(in, out, g, a, x0, x1, xb0, xb1, st, ch, fb, kn, het);
	});
	return true;
}

#if GCMX_TX2_BLKT
// 8192 x 8 x 2 start / end times and 8192 HW_IDs of the last launch, then zeroed
#if GCMX_FMA
extern "C" int gcmx_diag_blk_fma(unsigned long long* t, unsigned* hw) {
#else
extern "C" int gcmx_diag_blk(unsigned long long* t, unsigned* hw) {
#endif
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	if (hipMemcpyFromSymbol(t, HIP_SYMBOL(g_tx2_blk), sizeof(g_tx2_blk)) != hipSuccess) return -1;
	if (hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_tx2_hw), sizeof(g_tx2_hw)) != hipSuccess) return -1;
	static unsigned long long zero[kBlkMax][8][2];
	return hipMemcpyToSymbol(HIP_SYMBOL(g_tx2_blk), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

bool launch_fused_xyz(const double* in, double* out, const Geo& g, const IsoAxis* a, int x0,
                      int x1, hipStream_t st, int chunk, const FaceBC* faces, const char** kname,
                      const HetMaterials* het, int xb0, int xb1) {
	const char* dummy = nullptr;
	const char** kn = kname ? kname : &dummy;
	if (!fused_supported(g) || x1 <= x0) return false;
	if (xb1 > xb0 && (xb0 < x1 || xb1 > g.sizes[0])) return false;  // range B after range A
	if (het && !het_supported(g)) return false;
	// the z split takes rows longer than 512 (and GCMX_ZS_PART's): uniform medium,
	// floor(q) = 0 -- then with face conditions and the folded ODE too
	const bool zs = !het && zs_admissible(g, a);
	if (faces && faces->on && !(fused_faces_supported(g) && (g.sizes[2] <= 512 || zs))) return false;
	if (faces && faces->ode_on && !(g.bs <= 2 && (g.sizes[2] <= 512 || zs))) return false;  // k_fused_xyz has no epilogue
	if (zs) {
		const int P = zs_part(g);
		const bool fc = faces && faces->on;
		auto go = [&](auto F) {
			constexpr bool FC = decltype(F)::value;
			if (g.bs == 1) P == 256 ? launch_zs<1, 256, FC>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn)
			               : launch_zs<1, 512, FC>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn);
			else P == 256 ? launch_zs<2, 256, FC>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn)
			              : launch_zs<2, 512, FC>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn);
		};
		if (fc) go(std::true_type{});
		else go(std::false_type{});
		return true;
	}
	switch (g.bs) {
	case 1: return launch_xyz_bs<1>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn, het);
	case 2: return launch_xyz_bs<2>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn, het);
	case 3: return launch_xyz_bs<3>(in, out, g, a, x0, x1, xb0, xb1, st, chunk, faces, kn, het);
	default: return false;
	}
}

}  // namespace GCMX_BUILD_NS

#if !GCMX_FMA
// CUs the one-pass step leaves free while it covers planes [x0, x1) in one
// round (the slab interior of the boundary-first schedule); 0 when its blocks
// fill every CU or it takes more than one round, -1 when k_step_tx2 does not run.
int step_free_cus(const Geo& g, int x0, int x1, int req_chunk, int cus_in) {
	const int Z = g.sizes[2];
	if (!fused_supported(g) || g.bs > 2 || Z > 512 || x1 <= x0) return -1;
	const int ZT = row_lanes(Z);
	const int per_cu = 512 / ZT, cus = cus_in > 0 ? cus_in : GCMX_BUILD_NS::device_cus();
	const int npair = (x1 - x0 + ((g.gx0 + x0) & 1) + 1) / 2;
	const int chunk = GCMX_BUILD_NS::tx2_chunk_for(g.sizes[1], npair, req_chunk, cus * per_cu);
	const long long blocks = (long long)((g.sizes[1] + chunk - 1) / chunk) * npair;
	const long long slots = (long long)cus * per_cu;
	return blocks >= slots ? 0 : (int)((slots - blocks) / per_cu);
}

int zs_part(const Geo& g) {
	// GCMX_ZS_PART=256 (tuning): rows of 512 and more cut into 256-lane parts
	static const int env = [] {
		const char* e = std::getenv("GCMX_ZS_PART");
		return e ? std::atoi(e) : 0;
	}();
	const int Z = g.sizes[2];
	if (g.D != 3 || g.bs > 2) return 0;
	if (env == 256 && Z >= 512 && Z % 256 == 0) return 256;
	return Z > 512 && Z % 512 == 0 ? 512 : 0;
}


bool het_supported(const Geo& g) {
	const int Z = g.sizes[2];
	return fused_supported(g) && g.bs <= 2 && (Z == 64 || Z == 128 || Z == 256 || Z == 512);
}

bool fused_faces_supported(const Geo& g) {
	return fused_supported(g) && g.bs <= 2 && (g.sizes[2] <= 512 || zs_part(g) > 0) && g.sizes[1] >= 2 * g.bs + 2 &&
	       g.sizes[2] >= 2 * g.bs + 2;
}

bool zs_admissible(const Geo& g, const IsoAxis* a) {
	if (zs_part(g) <= 0) return false;
	for (int s = 0; s < 3; s++)
		if (a[s].kf1 != 0 || a[s].kf2 != 0) return false;
	return GCMX_BUILD_NS::same_axis(a[0], a[1]) && GCMX_BUILD_NS::same_axis(a[0], a[2]);
}

#endif

}  // namespace gcmx
