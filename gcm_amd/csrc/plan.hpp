// plan.hpp -- which kernel family runs a step, whether the y/z faces are formed
// inside the pass and whether the Maxwell ODE rides in its stores: one pure
// function of plain data, so the decision can be read and tested without a GPU
// (tests/plan_check.cpp).  gcmx.hip fills PlanFacts from a context (facts_of)
// and executes the StepPlan; nothing else decides.  DESIGN.md §3.12 has the table.
#pragma once
#include <cstdint>

#include "../../include/gcmx.h"

namespace gcmx {

// What the matrices' structure admits (refresh_fast): at most one pattern.
enum class Medium : uint8_t {
	General,   // no pattern: k_stage_generic, or the table kernel of the 2-D step
	Iso3,      // 3-D, one material, no ids, the isotropic structure
	Iso2,      // 2-D, one material, no ids, the ElasticModel<2> structure
	IsoHet,    // 3-D, per-node ids, every material isotropic (k_step_tx2 HET)
	Ortho,     // 3-D, one material, no ids, unrotated orthotropic (k_step_ortho)
	OrthoHet,  // 3-D, per-node ids, every material orthotropic (k_step_ortho HET)
	Acoustic,  // acoustic context, one material, no ids, the acoustic structure
};

constexpr int kPlanHetMaxMaterials = 32;  // launch.hpp's kHetMaxMaterials (asserted equal in gcmx.hip)

// Everything the decision reads.  The geometry predicates are launch.hpp's,
// evaluated by the caller.
struct PlanFacts {
	int D, bs, Y, Z, n_mat;
	gcmx_model model;
	Medium medium;
	bool tau_ok;   // this tau's feet lie where the medium's one-pass kernel reads them (build_tables)
	bool has_ids;  // per-node material ids are set
	gcmx_path path;  // forced by gcmx_set_kernel_path
	bool ghosts_touched;
	unsigned faces_written;  // bit 2*axis + side: a face fill wrote these ghosts
	bool has_halo;
	bool fused_supported, fused_faces_supported, zs_admissible, het_supported, ortho_supported,
	    ortho_het_supported, acoustic_supported, step2d_supported, step2d_iso_supported, fast_layout_ok;
};

enum class FaceSource : uint8_t { None, Faces, Map };  // gcmx_step; whole faces; a gcmx_face_map

struct StepRequest {
	FaceSource source;
	unsigned on;         // faces with a condition, bit 2*axis + side
	bool yz_pressure;    // a y or z face (2-D: a y face) sets PRESSURE
	bool ode;            // the Maxwell ODE follows the step
	int n_factors;       // its factors (one per material)
};

enum class StepKind : uint8_t { Stages, Step2d, Tx2, Ortho, Acoustic };

struct StepPlan {
	StepKind kind;       // Tx2: k_step_tx2 / k_fused_xyz, homogeneous or HET
	bool faces_in_pass;  // x faces filled in memory up front, y/z faces formed by the one pass
	bool ode_folded;     // the ODE factor rides in the pass's store epilogue
};
inline bool operator==(const StepPlan& a, const StepPlan& b) {
	return a.kind == b.kind && a.faces_in_pass == b.faces_in_pass && a.ode_folded == b.ode_folded;
}

// The one-pass family the medium, the geometry, the forced path and the ghost
// state admit, before the per-step conditions (faces_written, tau_ok).
inline StepKind plan_admitted_kind(const PlanFacts& f) {
	// a forced per-stage path; ghost values that are not zero make the two time
	// layers differ in their ghosts, and a one-pass step leaves the state in the other layer
	if ((f.path != GCMX_PATH_AUTO && f.path != GCMX_PATH_FUSED) || f.ghosts_touched) return StepKind::Stages;
	switch (f.medium) {
	case Medium::Acoustic:  // 3-D only; no X slabs are built for acoustic contexts
		return f.D == 3 && f.bs <= 3 && f.acoustic_supported && !f.has_halo ? StepKind::Acoustic : StepKind::Stages;
	case Medium::IsoHet:  // recognised only where het_supported holds
		return StepKind::Tx2;
	case Medium::OrthoHet:  // the homogeneous step's conditions, the HET instance set
		return f.bs <= 3 && f.ortho_het_supported ? StepKind::Ortho : StepKind::Stages;
	case Medium::Ortho:
		return f.bs <= 3 && f.ortho_supported ? StepKind::Ortho : StepKind::Stages;
	case Medium::Iso3:
		return f.D == 3 && f.bs <= 3 && f.fused_supported ? StepKind::Tx2 : StepKind::Stages;
	case Medium::Iso2:
	case Medium::General:
		// k_step2d: one elastic material, no X-slab exchange, a borderSize it is built for
		return f.D == 2 && f.model == GCMX_MODEL_ELASTIC && f.step2d_supported && !f.has_ids && f.n_mat == 1 &&
		               !f.has_halo
		           ? StepKind::Step2d
		           : StepKind::Stages;
	}
	return StepKind::Stages;
}

// gcmx_effective_path: what a plain step would run on the state as it stands.
inline gcmx_path plan_effective_path(const PlanFacts& f) {
	bool onepass = plan_admitted_kind(f) != StepKind::Stages;
	// k_step_tx2 takes a face step that refreshes the written faces, so the query
	// does not hold them against it; every other one-pass kernel needs zero y/z ghosts
	if (f.medium != Medium::Iso3 && f.medium != Medium::IsoHet) onepass = onepass && f.faces_written == 0;
	// a per-node medium's tau_ok is known only once a step built its tables: the
	// query ignores it (the step does not)
	if (f.medium != Medium::IsoHet && f.medium != Medium::OrthoHet) onepass = onepass && f.tau_ok;
	if (onepass) return GCMX_PATH_FUSED;
	// the per-stage kernels (isotropic, 3-D) address whole layers with 32-bit offsets
	const bool split = f.medium == Medium::Iso3 && f.D == 3 && f.bs <= 3 && f.path != GCMX_PATH_GENERIC && f.fast_layout_ok;
	return split ? GCMX_PATH_SPLIT : GCMX_PATH_GENERIC;
}

// gcmx_stage: the per-stage kernels of the split path, or k_stage_generic.
inline gcmx_path plan_stage_path(const PlanFacts& f) {
	// no per-stage kernels for the per-node, orthotropic and acoustic media; the split path's are 3-D only
	if (f.medium != Medium::Iso3 || f.D != 3 || !f.fast_layout_ok) return GCMX_PATH_GENERIC;
	return plan_effective_path(f) == GCMX_PATH_GENERIC ? GCMX_PATH_GENERIC : GCMX_PATH_SPLIT;
}

// One step call (after build_tables: tau_ok is per tau).
inline StepPlan plan_step(const PlanFacts& f, const StepRequest& r) {
	StepPlan p{StepKind::Stages, false, false};
	const StepKind k = plan_admitted_kind(f);
	if (k == StepKind::Stages) return p;
	// no face may hold ghosts written earlier but not refreshed now
	if ((f.faces_written & ~r.on) != 0) return p;
	// feet off the sides the kernel reads (tau <= 0, q = 0; per-node media: floor(q) != 0 or unequal axes)
	if (!f.tau_ok) return p;
	// rows longer than 512: only the z split (uniform medium, floor(q) = 0) forms faces and has the store epilogue
	const bool long_rows_ok = f.Z <= 512 || (!f.has_ids && f.zs_admissible);
	if (r.source != FaceSource::None) {
		// PRESSURE on a face formed in the pass: its trace needs components the pass does not form at ghosts
		if (r.yz_pressure) return p;
		switch (k) {
		case StepKind::Step2d:  // whole faces only; the isotropic kernel mirrors the inner columns (Y >= bs + 1)
			if (r.source != FaceSource::Faces || f.medium != Medium::Iso2 || !f.step2d_iso_supported || f.Y < f.bs + 1)
				return p;
			break;
		case StepKind::Tx2:
			if (!f.fused_faces_supported || !long_rows_ok) return p;
			break;
		default:  // k_step_ortho and k_step_acoustic form no faces
			return p;
		}
		p.faces_in_pass = true;
	}
	p.kind = k;
	// the ODE rides in k_step_tx2's store epilogue: over one material (one number), or over
	// per-node materials on the HET step (each node's own factor read from LDS)
	p.ode_folded = r.ode && k == StepKind::Tx2 && f.bs <= 2 && long_rows_ok &&
	               (f.has_ids ? f.medium == Medium::IsoHet && r.n_factors <= kPlanHetMaxMaterials : r.n_factors == 1);
	return p;
}

}  // namespace gcmx
