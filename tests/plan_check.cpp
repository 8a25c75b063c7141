// plan_check.cpp -- the step planner (gcm_amd/csrc/plan.hpp) over every
// combination of its inputs that a context can produce: the invariants the
// executor in gcmx.hip relies on, and the set of plans that can occur (printed,
// one per line, for tests/test_plan_cpu.py).  Built and run by that test with
// -fsanitize=address,undefined; needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "../gcm_amd/csrc/plan.hpp"
#include "../include/gcmx.h"

using namespace gcmx;

static long long g_checked = 0, g_failed = 0;
static const char* kind_name(StepKind k) {
	switch (k) {
	case StepKind::Stages: return "Stages";
	case StepKind::Step2d: return "Step2d";
	case StepKind::Tx2: return "Tx2";
	case StepKind::Ortho: return "Ortho";
	case StepKind::Acoustic: return "Acoustic";
	}
	return "?";
}

#define CHECK(cond, f, r)                                                                                         \
	do {                                                                                                          \
		if (!(cond)) {                                                                                            \
			if (g_failed++ < 20)                                                                                  \
				std::fprintf(stderr,                                                                              \
				             "FAILED %s: D %d model %d medium %d tau_ok %d bs %d Y %d Z %d ids %d n_mat %d path %d " \
				             "ghosts %d written %#x halo %d | source %d on %#x pressure %d ode %d factors %d\n",  \
				             #cond, f.D, (int)f.model, (int)f.medium, f.tau_ok, f.bs, f.Y, f.Z, f.has_ids, f.n_mat,  \
				             (int)f.path, f.ghosts_touched, f.faces_written, f.has_halo, (int)r.source, r.on,      \
				             r.yz_pressure, r.ode, r.n_factors);                                                  \
		}                                                                                                         \
	} while (0)

// What facts_of (gcmx.hip) cannot produce: the rules of refresh_fast, of the
// geometry predicates (kernels_*.hip) and of the ABI.
static bool reachable(const PlanFacts& f) {
	const bool ac = f.model == GCMX_MODEL_ACOUSTIC;
	// an acoustic context tries the acoustic pattern only, an elastic one never
	if (ac ? (f.medium != Medium::General && f.medium != Medium::Acoustic) : f.medium == Medium::Acoustic) return false;
	// the 3-D patterns, the 2-D pattern
	if ((f.medium == Medium::Iso3 || f.medium == Medium::IsoHet || f.medium == Medium::Ortho ||
	     f.medium == Medium::OrthoHet) && f.D != 3)
		return false;
	if (f.medium == Medium::Iso2 && f.D != 2) return false;
	// homogeneous patterns: one material, no ids; per-node ones: ids, 1..32 materials
	const bool homog = f.medium == Medium::Iso3 || f.medium == Medium::Iso2 || f.medium == Medium::Ortho ||
	                   f.medium == Medium::Acoustic;
	const bool pernode = f.medium == Medium::IsoHet || f.medium == Medium::OrthoHet;
	if (homog && (f.has_ids || f.n_mat != 1)) return false;
	if (pernode && (!f.has_ids || f.n_mat > kPlanHetMaxMaterials)) return false;
	// tau_ok is cleared only where build_tables checks sides: Ortho, Acoustic, the per-node media
	if (!f.tau_ok && (f.medium == Medium::General || f.medium == Medium::Iso3 || f.medium == Medium::Iso2)) return false;
	// recognition needs the kernel's geometry
	if (f.medium == Medium::Iso2 && !f.step2d_iso_supported) return false;
	if (f.medium == Medium::IsoHet && !f.het_supported) return false;
	// the geometry predicates imply one another
	if (f.step2d_iso_supported && !(f.step2d_supported && f.bs <= 3)) return false;
	if (f.step2d_supported && !(f.D == 2 && !ac)) return false;  // M == 5
	if (f.fused_supported && !(f.D == 3 && f.bs <= 3 && f.Z <= 1024)) return false;
	if (f.fast_layout_ok && !(f.D == 3 && f.bs <= 3)) return false;
	if (f.het_supported && !(f.fused_supported && f.bs <= 2 && f.Z <= 512)) return false;
	if (f.fused_faces_supported && !(f.fused_supported && f.bs <= 2)) return false;
	if (f.ortho_supported && !(f.fused_supported && !(f.bs >= 3 && f.Z > 512))) return false;
	if (f.ortho_het_supported && !f.ortho_supported) return false;
	if (f.acoustic_supported && !(f.fused_supported && ac)) return false;  // M == 4
	if (f.zs_admissible && !(f.medium == Medium::Iso3 && f.Z > 512 && f.fused_supported)) return false;
	// X slabs are refused for acoustic contexts and need dim >= 2
	if (f.has_halo && (ac || f.D < 2)) return false;
	// faces exist on the grid's axes only; below 3-D the z extent is 1
	if (f.faces_written >> (2 * f.D)) return false;
	if (f.D < 3 && f.Z != 1) return false;
	if (f.D == 3 && f.Z == 1) return false;
	return true;
}

static bool request_possible(const PlanFacts& f, const StepRequest& r) {
	if (r.on >> (2 * f.D)) return false;
	if (r.source == FaceSource::None && (r.on != 0 || r.yz_pressure)) return false;
	if (r.yz_pressure && (r.on >> 2) == 0) return false;  // some y/z face sets it
	if (r.ode && (f.model == GCMX_MODEL_ACOUSTIC || r.source == FaceSource::Map)) return false;  // refused / not offered
	if (r.n_factors != (r.ode ? f.n_mat : 0)) return false;  // one factor per material
	return true;
}

int main() {
	std::set<std::string> plans;
	const gcmx_model models[] = {GCMX_MODEL_ELASTIC, GCMX_MODEL_ACOUSTIC};
	const Medium media[] = {Medium::General, Medium::Iso3, Medium::Iso2, Medium::IsoHet,
	                        Medium::Ortho, Medium::OrthoHet, Medium::Acoustic};
	const gcmx_path paths[] = {GCMX_PATH_AUTO, GCMX_PATH_GENERIC, GCMX_PATH_SPLIT, GCMX_PATH_FUSED};
	const int zs[] = {1, 64, 512, 1024}, nmats[] = {1, 2, 33}, ys[] = {2, 9};
	const unsigned written[] = {0u, 1u, 4u, 0x30u, 0x3fu}, ons[] = {0u, 3u, 4u, 0x3cu, 0x3fu};
	PlanFacts f{};
	for (gcmx_model model : models)
	for (int D = 1; D <= 3; D++)
	for (Medium medium : media)
	for (int tau_ok = 0; tau_ok < 2; tau_ok++)
	for (int bs = 1; bs <= 4; bs++)
	for (int Z : zs)
	for (int Y : ys)
	for (int ids = 0; ids < 2; ids++)
	for (int n_mat : nmats)
	for (unsigned geo = 0; geo < (1u << 10); geo++) {
		f.model = model, f.D = D, f.medium = medium, f.tau_ok = tau_ok, f.bs = bs, f.Z = Z, f.Y = Y;
		f.has_ids = ids, f.n_mat = n_mat;
		f.fused_supported = geo & 1, f.fused_faces_supported = geo & 2, f.zs_admissible = geo & 4;
		f.het_supported = geo & 8, f.ortho_supported = geo & 16, f.ortho_het_supported = geo & 32;
		f.acoustic_supported = geo & 64, f.step2d_supported = geo & 128, f.step2d_iso_supported = geo & 256;
		f.fast_layout_ok = geo & 512;
		f.path = GCMX_PATH_AUTO, f.ghosts_touched = false, f.faces_written = 0, f.has_halo = false;
		if (!reachable(f)) continue;
		for (gcmx_path path : paths)
		for (int ghosts = 0; ghosts < 2; ghosts++)
		for (unsigned fw : written)
		for (int halo = 0; halo < 2; halo++) {
			f.path = path, f.ghosts_touched = ghosts, f.faces_written = fw, f.has_halo = halo;
			if (!reachable(f)) continue;
			const gcmx_path eff = plan_effective_path(f), stage = plan_stage_path(f);
			StepRequest none{FaceSource::None, 0, false, false, 0};
			CHECK(stage != GCMX_PATH_FUSED && stage != GCMX_PATH_AUTO, f, none);
			CHECK(eff != GCMX_PATH_AUTO, f, none);
			for (int source = 0; source < 3; source++)
			for (unsigned on : ons)
			for (int pressure = 0; pressure < 2; pressure++)
			for (int ode = 0; ode < 2; ode++) {
				const StepRequest r{(FaceSource)source, on, pressure != 0, ode != 0, ode ? n_mat : 0};
				if (!request_possible(f, r)) continue;
				const StepPlan p = plan_step(f, r);
				g_checked++;
				const bool onepass = p.kind != StepKind::Stages;
				// a one-pass kind only where the plain query admits it up to the faces this step refreshes
				PlanFacts refreshed = f;
				refreshed.faces_written &= ~r.on;
				if (f.medium == Medium::IsoHet || f.medium == Medium::OrthoHet) refreshed.tau_ok = true;  // the query ignores it
				CHECK(!onepass || plan_effective_path(refreshed) == GCMX_PATH_FUSED, f, r);
				CHECK(!onepass || r.source != FaceSource::None || eff == GCMX_PATH_FUSED, f, r);
				CHECK(!onepass || ((f.faces_written & ~r.on) == 0 && !f.ghosts_touched), f, r);
				CHECK(!p.faces_in_pass || ((p.kind == StepKind::Tx2 || p.kind == StepKind::Step2d) &&
				                           f.model == GCMX_MODEL_ELASTIC && !r.yz_pressure),
				      f, r);
				CHECK(p.faces_in_pass == (onepass && r.source != FaceSource::None), f, r);
				CHECK(!p.ode_folded || (r.ode && p.kind == StepKind::Tx2 && f.bs <= 2 &&
				                        ((!f.has_ids && r.n_factors == 1) ||
				                         (f.medium == Medium::IsoHet && f.tau_ok && r.n_factors <= 32))),
				      f, r);
				CHECK(p.kind != StepKind::Acoustic || (r.source == FaceSource::None && r.on == 0 && !f.has_halo && f.D == 3), f, r);
				CHECK((p.kind != StepKind::Ortho && p.kind != StepKind::Acoustic) || f.tau_ok, f, r);
				CHECK(!(p.kind == StepKind::Tx2 && f.medium == Medium::IsoHet) || f.tau_ok, f, r);
				CHECK(!(f.path == GCMX_PATH_GENERIC || f.path == GCMX_PATH_SPLIT) || !onepass, f, r);
				// the kernel family belongs to the medium and the dimension
				CHECK(p.kind != StepKind::Tx2 || ((f.medium == Medium::Iso3 || f.medium == Medium::IsoHet) && f.D == 3), f, r);
				CHECK(p.kind != StepKind::Ortho || ((f.medium == Medium::Ortho || f.medium == Medium::OrthoHet) && f.D == 3), f, r);
				CHECK(p.kind != StepKind::Acoustic || f.medium == Medium::Acoustic, f, r);
				CHECK(p.kind != StepKind::Step2d || (f.D == 2 && f.step2d_supported && r.source != FaceSource::Map), f, r);
				CHECK(plan_step(f, r) == p, f, r);  // a function of its arguments
				plans.insert(std::string(kind_name(p.kind)) + (p.faces_in_pass ? " faces" : " -") +
				             (p.ode_folded ? " ode" : " -"));
			}
		}
	}
	for (const std::string& s : plans) std::printf("plan %s\n", s.c_str());
	std::printf("checked %lld requests, %lld failed\n", g_checked, g_failed);
	return g_failed ? 1 : 0;
}
