// engine.cpp -- host mirror of the cubic engine (see engine.hpp for the map).
#include "engine.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

namespace gcm {

real Clock::time = 0;
real Clock::timeStep = 0;

void gcmxCheck(gcmx_status s, const char* what) {
	if (s != GCMX_OK)
		throw Exception(std::string(what) + ": " + gcmx_status_string(s) + ": " + gcmx_last_error());
}

// ------------------------------------------------------------ AbstractEngine --

AbstractEngine::AbstractEngine(const Task& task)
    : CourantNumber(task.globalSettings.CourantNumber), checkpoint(task.checkpoint) {
	Clock::setZero();
}

void AbstractEngine::saveState(const std::string&) const { throw Exception("saveState: only the cubic engine saves its state"); }
void AbstractEngine::loadState(const std::string&) { throw Exception("loadState: only the cubic engine loads a state"); }

std::string AbstractEngine::checkpointFile() const {
	if (checkpoint.stepsPerCheckpoint <= 0) return "";
	return (checkpoint.directory.empty() ? std::string(".") : checkpoint.directory) + "/checkpoint.gcmx";
}

void AbstractEngine::restoreClock(int steps_, real time, real timeStep) {
	steps = steps_;
	Clock::time = time;
	Clock::timeStep = timeStep;
	resumed = true;
}

// AbstractEngine.cpp:18-27
void AbstractEngine::afterConstruction(const Task& task) {
	Clock::timeStep = estimateTimeStep();
	requiredTime = Clock::TimeStep() * task.globalSettings.numberOfSnaps *
	               task.globalSettings.stepsPerSnap;
	if (task.globalSettings.numberOfSnaps <= 0) requiredTime = task.globalSettings.requiredTime;
	if (!(requiredTime > 0)) throw Exception("requiredTime must be > 0");
}

// AbstractEngine.cpp:30-46
void AbstractEngine::run() {
	// after loadState the saved run goes on: its step numbers, and no second
	// snapshot of the step it was saved at
	int step = resumed ? steps : 0;
	if (!resumed) writeSnapshots(step);
	resumed = false;
	const std::string file = checkpointFile();
	while (Clock::Time() < requiredTime) {
		Clock::timeStep = estimateTimeStep();
		nextTimeStep();
		step++;
		steps++;
		Clock::tickTack();
		writeSnapshots(step);
		if (!file.empty() && step % checkpoint.stepsPerCheckpoint == 0) saveState(file);
	}
	flushSnapshots();
}

void AbstractEngine::runSteps(int n) {
	for (int i = 0; i < n; i++) {
		Clock::timeStep = estimateTimeStep();
		nextTimeStep();
		steps++;
		Clock::tickTack();
	}
}

namespace cubic {

// ------------------------------------------------------------------ CubicGrid --

template <int D>
CubicGrid<D>::CubicGrid(size_t id_, const ConstructionPack& cp)
    : id(id_), borderSize(cp.borderSize), sizes(cp.sizes), start(cp.start), h(cp.h) {
	// CubicGrid.hpp:184-199 and calculateIndexMaker :202-225
	if (!(borderSize > 0)) throw Exception("CubicGrid: borderSize must be > 0");
	for (int i = 0; i < D; i++) {
		if (!(sizes[i] >= borderSize)) throw Exception("CubicGrid: sizes must be >= borderSize");
		if (!(h[i] > 0)) throw Exception("CubicGrid: h must be > 0");
	}
	const long long b2 = 2LL * borderSize;
	if (D == 1) {
		indexMaker[0] = 1;
	} else if (D == 2) {
		indexMaker[0] = b2 + sizes[D - 1];
		indexMaker[D - 1] = 1;
	} else {
		indexMaker[0] = (b2 + sizes[1 % D]) * (b2 + sizes[D - 1]);
		indexMaker[1 % D] = b2 + sizes[D - 1];
		indexMaker[D - 1] = 1;
	}
}

template <int D>
real CubicGrid<D>::getMinimalSpatialStep() const {
	real ans = std::numeric_limits<real>::max();
	for (int i = 0; i < D; i++)
		if (ans > h[i]) ans = h[i];
	return ans;
}

template <int D>
std::pair<typename CubicGrid<D>::IntD, typename CubicGrid<D>::IntD> CubicGrid<D>::aabb() const {
	IntD mx;
	for (int i = 0; i < D; i++) mx[i] = start[i] + sizes[i] - 1;
	return {start, mx};
}

/// Calls f(it) for every inner node in SlowXFastZ order (linal/Multiindex.hpp:99-118),
/// optionally restricted to it[axis] == fixed.
template <int D, class F>
static void forEachInner(const std::array<int, D>& sizes, F f, int axis = -1, int fixed = 0) {
	std::array<int, D> it{};
	std::array<int, D> lo{}, hi = sizes;
	if (axis >= 0) {
		lo[axis] = fixed;
		hi[axis] = fixed + 1;
	}
	it = lo;
	while (true) {
		f(it);
		int d = D - 1;
		for (; d >= 0; d--) {
			if (++it[d] < hi[d]) break;
			it[d] = lo[d];
		}
		if (d < 0) break;
	}
}

// -------------------------------------------------------------------- HipMesh --

template <int D>
HipMesh<D>::HipMesh(const Task& task, size_t id_, const typename CubicGrid<D>::ConstructionPack& cp,
                    int device_)
    : AbstractMesh<D>(id_, cp), device(device_) {
	const auto tb = task.bodies.find(id_);
	if (tb != task.bodies.end()) model_ = tb->second.modelId;
	gcmx_grid_desc desc{};
	desc.dim = D;
	desc.border_size = cp.borderSize;
	for (int i = 0; i < 3; i++) {
		desc.sizes[i] = i < D ? cp.sizes[i] : 1;
		desc.start[i] = i < D ? cp.start[i] : 0;
		desc.h[i] = i < D ? cp.h[i] : 0;
	}
	gcmxCheck(gcmx_create_model(&desc, model_ == Models::T::ACOUSTIC ? GCMX_MODEL_ACOUSTIC : GCMX_MODEL_ELASTIC,
	                            device, &ctx_), "gcmx_create_model");
}

template <int D>
HipMesh<D>::~HipMesh() {
	if (ownsCtx_) gcmx_destroy(ctx_);
}

// ---------------------------------------------------------------------- stacks --

/// Calls f(it) for every node of a grid of `sizes` INCLUDING bs ghost layers.
template <int D, class F>
static void forEachAll(const std::array<int, D>& sizes, int bs, F f) {
	std::array<int, D> it;
	for (int d = 0; d < D; d++) it[d] = -bs;
	while (true) {
		f(it);
		int d = D - 1;
		for (; d >= 0; d--) {
			if (++it[d] < sizes[d] + bs) break;
			it[d] = -bs;
		}
		if (d < 0) break;
	}
}

template <int D>
void HipMesh<D>::joinStack(const std::shared_ptr<HipMesh<D>>& stack, int axis, int offset) {
	if (stack_) throw Exception("the body is in a stack already");
	if (ownsCtx_) gcmx_destroy(ctx_);  // its device layers live in the stack
	ctx_ = stack->ctx_;
	ownsCtx_ = false;
	stack_ = stack;
	stackAxis_ = axis;
	stackOffset_ = offset;
}

// ------------------------------------------------------- set-up on the device --

gcmx_area deviceArea(const Area& area) {
	gcmx_area a{};
	if (dynamic_cast<const InfiniteArea*>(&area)) {
		a.kind = GCMX_AREA_INFINITE;
	} else if (const auto* b = dynamic_cast<const AxisAlignedBoxArea*>(&area)) {
		a.kind = GCMX_AREA_BOX;
		for (int i = 0; i < 3; i++) {
			a.p[i] = b->min[i];
			a.p[3 + i] = b->max[i];
		}
	} else if (const auto* s = dynamic_cast<const SphereArea*>(&area)) {
		a.kind = GCMX_AREA_SPHERE;
		a.p[0] = s->radius;
		for (int i = 0; i < 3; i++) a.p[1 + i] = s->center[i];
	} else if (const auto* c = dynamic_cast<const StraightBoundedCylinderArea*>(&area)) {
		a.kind = GCMX_AREA_CYLINDER;
		a.p[0] = c->radius;
		for (int i = 0; i < 3; i++) {
			a.p[1 + i] = c->begin[i];
			a.p[4 + i] = c->end[i];
			a.p[7 + i] = c->axis[i];
		}
	} else {
		throw Exception("set-up on the device: an Area of a kind the device does not know");
	}
	return a;
}

namespace {

std::vector<gcmx_area> deviceAreas(const std::vector<std::shared_ptr<Area>>& areas) {
	std::vector<gcmx_area> out;
	for (const auto& a : areas) {
		if (!a) throw Exception("set-up on the device: a condition without an area");
		out.push_back(deviceArea(*a));
	}
	return out;
}

/// gcmx_setup_state for the (area, vector) pairs of a body; no pair: the layer
/// keeps the zeros it was created with.
template <int D>
void deviceInitialState(gcmx_ctx* ctx, const gcmx_setup_box* box, const SetUpLists<D>& ls) {
	if (ls.initial.empty()) return;
	std::vector<gcmx_area> areas;
	std::vector<real> vectors;
	for (const auto& ic : ls.initial) {
		if (!ic.first) throw Exception("set-up on the device: a condition without an area");
		areas.push_back(deviceArea(*ic.first));
		vectors.insert(vectors.end(), ic.second.begin(), ic.second.begin() + ls.st.M);
	}
	gcmxCheck(gcmx_setup_state(ctx, box, (int)areas.size(), areas.data(), vectors.data()), "gcmx_setup_state");
}

/// The ids (entries of `idOf`) that occur in the box, as flags.
std::vector<int> deviceCensus(gcmx_ctx* ctx, const gcmx_setup_box* box, const std::vector<gcmx_area>& areas,
                              const std::vector<uint8_t>& idOf, size_t nIds) {
	uint32_t mask[8] = {};
	gcmxCheck(gcmx_setup_census(ctx, box, (int)areas.size(), areas.data(), idOf.data(), mask), "gcmx_setup_census");
	std::vector<int> used(nIds, 0);
	for (size_t v = 0; v < nIds && v < 256; v++) used[v] = (mask[v >> 5] >> (v & 31)) & 1;
	return used;
}

}  // namespace

// ----------------------------------------------------------------- placement --

template <int D>
typename HipMesh<D>::PlacedBox HipMesh<D>::placeBox(const IntD& boxMin, const IntD& boxMax, int reach,
                                                    const char* refusal) const {
	for (int d = 0; d < D; d++)
		if (boxMin[d] < -reach || boxMax[d] > this->sizes[d] + reach) throw Exception(refusal);
	const IntD lo = inContext(boxMin), hi = inContext(boxMax);
	PlacedBox p;
	std::copy(lo.begin(), lo.end(), p.lo);
	std::copy(hi.begin(), hi.end(), p.hi);
	return p;
}

template <int D>
gcmx_setup_box HipMesh<D>::setupBox() const {
	const PlacedBox p = placeBox(IntD{}, this->sizes, 0, "setupBox");
	gcmx_setup_box b{};
	for (int d = 0; d < 3; d++) {
		b.min[d] = p.lo[d];
		b.max[d] = p.hi[d];
		b.start[d] = d < D ? this->start[d] : 0;
	}
	return b;
}

// -------------------------------------------------------------------- set-up --

template <int D, class Matrices>
static typename MaterialTable<D>::Entry materialEntry(const Matrices& m, real tau0) {
	typename MaterialTable<D>::Entry e{};
	for (int s = 0; s < D; s++) {
		e.U[s] = m.m[s].U.data();
		e.U1[s] = m.m[s].U1.data();
		e.L[s] = m.m[s].L.data();
	}
	e.bits = &m;
	e.nBits = sizeof(m);
	e.tau0 = tau0;
	e.maximalEigenvalue = m.getMaximalEigenvalue();
	return e;
}

template <int D>
MaterialTable<D> buildMaterialTable(const std::vector<SetUpLists<D>>& lists, bool share) {
	typedef typename MaterialTable<D>::Entry Entry;
	MaterialTable<D> t;
	t.entryOf.resize(lists.size());
	for (size_t k = 0; k < lists.size(); k++) {
		const HostState<D>& st = lists[k].st;
		t.M = st.M;
		for (size_t c = 0; c < st.numberOfConditions(); c++) {
			const Entry e = st.model == Models::T::ACOUSTIC ? materialEntry<D>(st.acousticMatrices[c], st.tau0[c])
			                                                : materialEntry<D>(st.matrices[c], st.tau0[c]);
			int found = -1;
			for (size_t i = 0; share && i < t.entries.size() && found < 0; i++) {
				const Entry& o = t.entries[i];
				if (o.nBits == e.nBits && std::memcmp(o.bits, e.bits, e.nBits) == 0 &&
				    std::memcmp(&o.tau0, &e.tau0, sizeof(real)) == 0)
					found = (int)i;
			}
			if (found < 0) {
				found = (int)t.entries.size();
				t.entries.push_back(e);
			}
			t.entryOf[k].push_back(found);
		}
	}
	// (a lone body cannot get here: buildSetUpLists holds it to 255 conditions)
	if (t.entries.size() > 255) throw Exception("a stack holds at most 255 materials");
	return t;
}

template <int D>
std::vector<int> HipMesh<D>::sendMaterials(const MaterialTable<D>& table, const std::vector<int>& used) {
	const size_t n = table.entries.size(), M = (size_t)table.M;
	std::vector<int> dev(n, -1);
	int nUsed = 0;
	for (size_t e = 0; e < n; e++)
		if (used[e]) dev[e] = nUsed++;
	std::vector<real> U((size_t)nUsed * D * M * M), U1(U.size()), L((size_t)nUsed * D * M);
	deviceTau0_.assign(nUsed, 0);
	for (size_t e = 0; e < n; e++) {
		if (dev[e] < 0) continue;
		deviceTau0_[dev[e]] = table.entries[e].tau0;
		for (int s = 0; s < D; s++) {
			const size_t o = (size_t)dev[e] * D + s;
			std::copy_n(table.entries[e].U[s], M * M, U.begin() + o * M * M);
			std::copy_n(table.entries[e].U1[s], M * M, U1.begin() + o * M * M);
			std::copy_n(table.entries[e].L[s], M, L.begin() + o * M);
		}
	}
	gcmxCheck(gcmx_set_materials(ctx_, nUsed, U.data(), U1.data(), L.data()), "gcmx_set_materials");
	return dev;
}

/// What differs between the set-up on the host and on the device: the node loops.
template <int D>
struct HipMesh<D>::NodePass {
	HipMesh<D>& owner;  // the mesh of the context
	const std::vector<HipMesh<D>*>& members;
	const std::vector<SetUpLists<D>>& lists;
	const MaterialTable<D>& table;
	NodePass(HipMesh<D>& o, const std::vector<HipMesh<D>*>& m, const std::vector<SetUpLists<D>>& l,
	         const MaterialTable<D>& t)
	    : owner(o), members(m), lists(l), table(t) {}
	virtual ~NodePass() = default;
	/// Per table entry: whether an inner node has it.
	virtual std::vector<int> census() = 0;
	/// Ids (where more than one material went to the device) and state, given
	/// entry -> device id; an unused entry's nodes -- ghosts only -- take id 0.
	virtual void place(const std::vector<int>& dev) = 0;
};

/// The node arrays of the context on the host, one gcmx_set_material_ids and one
/// gcmx_upload: every member's inner nodes and its ghost layers on the other axes;
/// along the stack axis a member's ghost layers at a contact are its neighbour's
/// inner layers (the stack's own ghosts only at its ends).
template <int D>
struct HipMesh<D>::HostNodePass : NodePass {
	using NodePass::NodePass;
	std::vector<real> pde;
	std::vector<uint8_t> ids;  // table entries, then device ids
	std::vector<int> census() override {
		const HipMesh<D>& owner = this->owner;
		std::vector<int> used(this->table.entries.size(), 0);
		pde.assign((size_t)owner.sizeOfAllNodes() * this->table.M, 0.0);
		ids.assign((size_t)owner.sizeOfAllNodes(), 0);
		for (size_t k = 0; k < this->members.size(); k++) {
			HipMesh<D>& mb = *this->members[k];
			const bool first = k == 0, last = k + 1 == this->members.size();
			const std::vector<int>& entryOf = this->table.entryOf[k];
			std::vector<uint8_t> cond((size_t)mb.sizeOfAllNodes(), 0);
			applySetUpLists<D>(this->lists[k], mb, cond, owner, mb.inContext(IntD{}), pde);
			const int a = mb.stackAxis_;
			forEachAll<D>(mb.sizes, mb.borderSize, [&](const IntD& it) {
				if (a >= 0 && ((it[a] < 0 && !first) || (it[a] >= mb.sizes[a] && !last))) return;
				const int e = entryOf[cond[(size_t)mb.getIndex(it)]];
				ids[(size_t)owner.getIndex(mb.inContext(it))] = (uint8_t)e;
				bool inner = true;
				for (int d = 0; d < D; d++) inner = inner && it[d] >= 0 && it[d] < mb.sizes[d];
				if (inner) used[(size_t)e] = 1;
			});
			// the snapshots' material array: condition indices, not device ids
			if (entryOf.size() > 1) mb.matIdAll_ = std::move(cond);
		}
		return used;
	}
	void place(const std::vector<int>& dev) override {
		if (this->owner.deviceTau0_.size() > 1) {
			for (auto& e : ids) e = (uint8_t)std::max(0, dev[e]);
			gcmxCheck(gcmx_set_material_ids(this->owner.ctx_, ids.data()), "gcmx_set_material_ids");
		}
		gcmxCheck(gcmx_upload(this->owner.ctx_, pde.data()), "gcmx_upload");
	}
};

/// Census, ids and state on the device, once per member over the member's box of
/// the context with its own start: the context's ghosts and the contact layers
/// need nothing beyond the members' inner nodes.  No gcmx_upload, and no host
/// array the size of the grid; a member's ids wait on the device until a snapshot
/// asks for them (fetchMaterialIds).
template <int D>
struct HipMesh<D>::DeviceNodePass : NodePass {
	using NodePass::NodePass;
	std::vector<std::vector<gcmx_area>> areas;
	std::vector<gcmx_setup_box> boxes;
	std::vector<int> census() override {
		std::vector<int> used(this->table.entries.size(), 0);
		for (size_t k = 0; k < this->members.size(); k++) {
			areas.push_back(deviceAreas(this->lists[k].materialAreas));
			boxes.push_back(this->members[k]->setupBox());
			const std::vector<int>& entryOf = this->table.entryOf[k];
			const std::vector<int> mine = deviceCensus(this->owner.ctx_, &boxes[k], areas[k],
			                                           std::vector<uint8_t>(entryOf.begin(), entryOf.end()), used.size());
			for (size_t e = 0; e < used.size(); e++) used[e] = used[e] || mine[e];
		}
		return used;
	}
	void place(const std::vector<int>& dev) override {
		gcmx_ctx* ctx = this->owner.ctx_;
		for (size_t k = 0; k < this->members.size(); k++) {
			HipMesh<D>& mb = *this->members[k];
			const std::vector<int>& entryOf = this->table.entryOf[k];
			if (this->owner.deviceTau0_.size() > 1) {
				std::vector<uint8_t> idOf;
				for (int e : entryOf) idOf.push_back((uint8_t)std::max(0, dev[(size_t)e]));
				gcmxCheck(gcmx_setup_material_ids(ctx, &boxes[k], (int)areas[k].size(), areas[k].data(), idOf.data()),
				          "gcmx_setup_material_ids");
			}
			deviceInitialState<D>(ctx, &boxes[k], this->lists[k]);
			if (entryOf.size() < 2) continue;
			mb.idsOnDevice_ = true;  // the snapshotters' material array: from the device on first use
			mb.materialAreas_ = this->lists[k].materialAreas;
			mb.conditionOfDeviceId_.assign(256, -1);
			for (size_t c = 0; c < entryOf.size(); c++) {
				const int d = dev[(size_t)entryOf[c]];
				if (d < 0) continue;
				int& slot = mb.conditionOfDeviceId_[(size_t)d];
				slot = slot == -1 ? (int)c : -2;  // two conditions of one material: the device cannot tell them apart
			}
		}
	}
};

template <int D>
void HipMesh<D>::markSetUp() {
	if (pdeIsSetUp) throw Exception("setUpPde called twice");
	pdeIsSetUp = true;
}

template <int D>
SetUpLists<D> HipMesh<D>::setUpMember(const Task& task) {
	markSetUp();
	SetUpLists<D> ls = buildSetUpLists<D>(task, *this);
	if (ls.st.model != model_) throw Exception("the body's model changed after its mesh was created");
	maximalEigenvalue = ls.st.maximalEigenvalue;  // over all its conditions, used or not: the time step reads it
	materialNumbers_ = ls.st.materialNumber;
	return ls;
}

template <int D>
void HipMesh<D>::setUp(const std::vector<HipMesh<D>*>& members, const std::vector<SetUpLists<D>>& lists, bool onDevice) {
	const bool stack = members.front() != this;  // or this mesh itself, as a stack of one
	if (stack) markSetUp();
	// a stack of one material stays homogeneous (the non-HET one-pass step); a lone
	// body keeps one device material per condition that holds nodes
	const MaterialTable<D> table = buildMaterialTable<D>(lists, stack);
	std::unique_ptr<NodePass> pass;
	if (onDevice) pass.reset(new DeviceNodePass(*this, members, lists, table));
	else pass.reset(new HostNodePass(*this, members, lists, table));
	const std::vector<int> dev = sendMaterials(table, pass->census());
	if (stack)  // the stack mesh's own eigenvalue: over the entries in use
		for (size_t e = 0; e < dev.size(); e++)
			if (dev[e] >= 0) maximalEigenvalue = std::fmax(maximalEigenvalue, table.entries[e].maximalEigenvalue);
	pass->place(dev);
}

// DefaultMesh::setUpPde (DefaultMesh.hpp:60-66): a lone body is a stack of one.
template <int D>
void HipMesh<D>::setUpPde(const Task& task) {
	std::vector<SetUpLists<D>> lists;
	lists.push_back(setUpMember(task));
	setUp({this}, lists, task.cubicGrid.setUpOnDevice);
}

template <int D>
void HipMesh<D>::fetchMaterialIds() const {
	idsOnDevice_ = false;
	const HipMesh<D>& owner = stack_ ? *stack_ : *this;  // whose context holds the ids
	std::vector<uint8_t> all((size_t)owner.sizeOfAllNodes());
	gcmxCheck(gcmx_download_material_ids(ctx_, all.data()), "gcmx_download_material_ids");
	matIdAll_.assign((size_t)this->sizeOfAllNodes(), 0);
	forEachInner<D>(this->sizes, [&](const IntD& it) {
		int c = conditionOfDeviceId_[all[(size_t)owner.getIndex(inContext(it))]];
		if (c == -2) {  // MaterialsCondition::apply for this node on the host
			const Real3 x = this->coords(it);
			for (size_t k = 0; k < materialAreas_.size(); k++)
				if (materialAreas_[k]->contains(x)) c = (int)k;
		}
		if (c < 0) throw Exception("a node's device material id names no material condition");
		matIdAll_[(size_t)this->getIndex(it)] = (uint8_t)c;
	});
}

template <int D>
typename CubicGrid<D>::ConstructionPack constructionPack(const Task& task, size_t id) {
	typename CubicGrid<D>::ConstructionPack cp;
	cp.borderSize = task.cubicGrid.borderSize;
	if ((int)task.cubicGrid.h.size() != D) throw Exception("h has the wrong size");
	const auto& cube = task.cubicGrid.cubics.at(id);
	if ((int)cube.sizes.size() != D || (int)cube.start.size() != D)
		throw Exception("cube sizes/start have the wrong size");
	for (int i = 0; i < D; i++) {
		cp.h[i] = task.cubicGrid.h[i];
		cp.sizes[i] = cube.sizes[i];
		cp.start[i] = cube.start[i];
	}
	return cp;
}

// DefaultMesh::setUpPde's host half (DefaultMesh.hpp:60-66): everything before
// the data would be stored, without touching a GPU.
template <int D>
HostState<D> buildHostState(const Task& task, const CubicGrid<D>& grid) {
	SetUpLists<D> ls = buildSetUpLists<D>(task, grid);
	std::vector<real> pde((size_t)grid.sizeOfAllNodes() * ls.st.M, 0.0);
	std::vector<uint8_t> matId((size_t)grid.sizeOfAllNodes(), 0);
	applySetUpLists<D>(ls, grid, matId, grid, std::array<int, D>{}, pde);
	ls.st.pde = std::move(pde);
	ls.st.matId = std::move(matId);
	return std::move(ls.st);
}

template <int D>
void applySetUpLists(const SetUpLists<D>& ls, const CubicGrid<D>& grid, std::vector<uint8_t>& matId,
                     const CubicGrid<D>& layer, const std::array<int, D>& shift, std::vector<real>& pde) {
	const int M = ls.st.M;
	// ---- MaterialsCondition::apply, the node loop (MaterialsCondition.hpp:23-36)
	forEachInner<D>(grid.sizes, [&](const std::array<int, D>& it) {
		const Real3 x = grid.coords(it);
		for (size_t c = 0; c < ls.materialAreas.size(); c++)
			if (ls.materialAreas[c]->contains(x)) matId[(size_t)grid.getIndex(it)] = (uint8_t)c;
	});
	// ---- InitialCondition::apply, the node loop (InitialCondition.hpp:23-88)
	forEachInner<D>(grid.sizes, [&](const std::array<int, D>& it) {
		const Real3 x = grid.coords(it);
		std::array<int, D> at = it;
		for (int d = 0; d < D; d++) at[d] += shift[d];
		real* v = &pde[(size_t)layer.getIndex(at) * M];
		for (int c = 0; c < M; c++) v[c] = 0;
		for (const auto& ic : ls.initial)
			if (ic.first->contains(x))
				for (int c = 0; c < M; c++) v[c] += ic.second[c];
	});
}

template <int D>
SetUpLists<D> buildSetUpLists(const Task& task, const CubicGrid<D>& grid) {
	constexpr int MX = pdeSize(D);  // the elastic vector; the acoustic one (D + 1) is no longer
	SetUpLists<D> ls;
	HostState<D>& st = ls.st;
	const auto body = task.bodies.find(grid.id);
	const Models::T model = body != task.bodies.end() ? body->second.modelId : Models::T::ELASTIC;
	const bool acoustic = model == Models::T::ACOUSTIC;
	const int M = pdeSizeOf(model, D);
	st.model = model;
	st.M = M;
	auto& matrices = st.matrices;

	// ---- MaterialsCondition::apply (util/task/MaterialsCondition.hpp:23-36, 70-91)
	// Body::materialId picks the kind every condition of the body is built with
	// (the reference's factory choice, Engine.cpp:155-189)
	typedef Task::MaterialCondition MC;
	struct Cond {
		std::shared_ptr<Area> first;
		MC::Material iso;
		MC::Orthotropic ortho;
	};
	std::vector<Cond> conds;
	const auto& mc = task.materialConditions;
	const Materials::T kind = body != task.bodies.end() ? body->second.materialId : Materials::T::ISOTROPIC;
	if (mc.type == MC::Type::BY_AREAS) {
		conds.push_back({std::make_shared<InfiniteArea>(), mc.byAreas.defaultMaterial, mc.byAreas.defaultOrthotropic});
		for (const auto& m : mc.byAreas.materials) conds.push_back({m.area, m.material, m.orthotropic});
	} else {
		const auto i = mc.byBodies.bodyMaterialMap.find(grid.id);
		const auto o = mc.byBodies.bodyOrthotropicMap.find(grid.id);
		if (i == mc.byBodies.bodyMaterialMap.end() && o == mc.byBodies.bodyOrthotropicMap.end())
			throw std::out_of_range("no material for this body");
		conds.push_back({std::make_shared<InfiniteArea>(),
		                 i != mc.byBodies.bodyMaterialMap.end() ? i->second : nullptr,
		                 o != mc.byBodies.bodyOrthotropicMap.end() ? o->second : nullptr});
	}
	if (conds.size() > 255) throw Exception("at most 255 material conditions per body");
	if (acoustic && kind != Materials::T::ISOTROPIC) throw Exception("acoustic bodies take isotropic materials only");
	if (acoustic) st.acousticMatrices.assign(conds.size(), AcousticMatrices<D>());
	else matrices.assign(conds.size(), GcmMatrices<D>());
	st.tau0.assign(conds.size(), 0);
	for (size_t c = 0; c < conds.size(); c++) {
		if (acoustic) {  // ISOTROPIC x ACOUSTIC: rho and lambda only, mu may be 0
			if (conds[c].ortho) throw Exception("orthotropic material in an ACOUSTIC body");
			if (!conds[c].iso) throw Exception("material condition without a material");
			AcousticModel<D>::constructGcmMatrices(st.acousticMatrices[c], *conds[c].iso);
			st.tau0[c] = conds[c].iso->tau0;
			st.materialNumber.push_back(conds[c].iso->materialNumber);
		} else if (kind == Materials::T::ORTHOTROPIC) {
			const MC::Orthotropic m = MC::orthotropicOf(conds[c].iso, conds[c].ortho);
			if (!m) throw Exception("material condition without a material");
			ElasticModel<D>::constructGcmMatrices(matrices[c], *m);
			st.tau0[c] = m->tau0;
			st.materialNumber.push_back(m->materialNumber);
		} else {
			if (conds[c].ortho) throw Exception("orthotropic material in an ISOTROPIC body (Body::materialId)");
			if (!conds[c].iso) throw Exception("material condition without a material");
			ElasticModel<D>::constructGcmMatrices(matrices[c], *conds[c].iso);
			st.tau0[c] = conds[c].iso->tau0;
			st.materialNumber.push_back(conds[c].iso->materialNumber);
		}
	}
	for (const Cond& c : conds) ls.materialAreas.push_back(c.first);
	st.maximalEigenvalue = 0;
	for (const auto& m : matrices)
		st.maximalEigenvalue = std::fmax(st.maximalEigenvalue, m.getMaximalEigenvalue());
	for (const auto& m : st.acousticMatrices)
		st.maximalEigenvalue = std::fmax(st.maximalEigenvalue, m.getMaximalEigenvalue());

	// ---- InitialCondition::apply (util/task/InitialCondition.hpp:23-88)
	auto& ics = ls.initial;  // the first M entries
	for (const auto& v : task.initialCondition.vectors) {
		if ((int)v.list.size() != M) throw Exception("initial vector has the wrong size");
		std::array<real, MX> a{};
		std::copy(v.list.begin(), v.list.end(), a.begin());
		ics.push_back({v.area, a});
	}
	{
		// mcConditions.front().material; an S wave or a stress quantity on an acoustic
		// body throws, as the reference's map lookups would (Model.cpp:55-60)
		for (const auto& w : task.initialCondition.waves) {
			if (!(w.direction >= 0 && w.direction < D)) throw Exception("wave direction out of range");
			const int col = acoustic ? acousticWaveColumn(w.waveType) : waveColumn(D, w.waveType, kind);
			std::array<real, MX> tmp{};
			for (int r = 0; r < M; r++)
				tmp[r] = acoustic ? st.acousticMatrices.front().m[w.direction].U1[r * M + col]
				                  : matrices.front().m[w.direction].U1[r * M + col];
			const real current = getQuantityOf(model, D, w.quantity, tmp.data());
			if (current == 0) throw Exception("wave calibration quantity is zero");
			const real f = w.quantityValue / current;
			for (int r = 0; r < M; r++) tmp[r] *= f;
			ics.push_back({w.area, tmp});
		}
	}
	for (const auto& q : task.initialCondition.quantities) {
		std::array<real, MX> tmp{};
		if (acoustic) setAcousticQuantity(D, q.physicalQuantity, q.value, tmp.data());
		else setQuantity(D, q.physicalQuantity, q.value, tmp.data());
		ics.push_back({q.area, tmp});
	}
	return ls;
}

template <int D>
std::vector<real> HipMesh<D>::pdeAll() const {
	// the all-nodes box; for a stack member its part of the stack (its ghost layers
	// at a contact: the neighbour's inner layers, as the contact copy leaves them)
	std::vector<real> out((size_t)this->sizeOfAllNodes() * pdeM());
	IntD lo, hi;
	for (int d = 0; d < D; d++) {
		lo[d] = -this->borderSize;
		hi[d] = this->sizes[d] + this->borderSize;
	}
	readBox(lo, hi, out.data());
	return out;
}

template <int D>
void HipMesh<D>::readBox(const IntD& boxMin, const IntD& boxMax, real* aos, size_t stageBytes) const {
	const PlacedBox p = placeBox(boxMin, boxMax, this->borderSize, "readBox: box outside the nodes of the mesh");
	gcmxCheck(gcmx_read_box(ctx_, p.lo, p.hi, aos, stageBytes), "gcmx_read_box");
}

template <int D>
void HipMesh<D>::writeBox(const IntD& boxMin, const IntD& boxMax, const real* aos, size_t stageBytes) {
	const PlacedBox p = placeBox(boxMin, boxMax, 0, "writeBox: only inner nodes can be written");
	gcmxCheck(gcmx_write_box(ctx_, p.lo, p.hi, aos, stageBytes), "gcmx_write_box");
}

template <int D>
std::array<real, HipMesh<D>::M> HipMesh<D>::pde(const IntD& it) const {
	const int m = pdeM();
	std::vector<int> components;
	for (int c = 0; c < m; c++) components.push_back(GCMX_Q_COMPONENT(c));
	const std::vector<real> got = gather(*nodeList({it}), components);
	std::array<real, M> v{};
	for (int c = 0; c < m; c++) v[c] = got[(size_t)c];
	return v;
}

// -------------------------------------------------------------- observation --

template <int D>
std::shared_ptr<typename HipMesh<D>::NodeList> HipMesh<D>::nodeList(const std::vector<IntD>& nodes) const {
	std::vector<int> flat;
	flat.reserve(nodes.size() * D);
	for (const IntD& it : nodes) {
		IntD next = it;
		for (int d = 0; d < D; d++) next[d]++;
		const PlacedBox p = placeBox(it, next, 0, "nodeList: only inner nodes can be observed");
		flat.insert(flat.end(), p.lo, p.lo + D);
	}
	auto list = std::make_shared<NodeList>();
	gcmxCheck(gcmx_node_list_create(ctx_, (int)nodes.size(), flat.data(), &list->handle), "gcmx_node_list_create");
	list->size = nodes.size();
	return list;
}

template <int D>
void HipMesh<D>::snapshotArrays(const IntD& boxMin, const IntD& boxMax, const std::vector<int>& quantities,
                                float* velocity, float* values) const {
	const PlacedBox p = placeBox(boxMin, boxMax, 0, "snapshotArrays: only inner nodes can be observed");
	gcmxCheck(gcmx_snapshot_box(ctx_, p.lo, p.hi, velocity ? 1 : 0, (int)quantities.size(), quantities.data(), velocity,
	                            values),
	          "gcmx_snapshot_box");
}

template <int D>
void HipMesh<D>::snapshotArrays(const IntD& boxMin, const IntD& boxMax, const IntD& stride,
                                const std::vector<int>& quantities, float* velocity, float* values) const {
	const PlacedBox p = placeBox(boxMin, boxMax, 0, "snapshotArrays: only inner nodes can be observed");
	int st[3] = {1, 1, 1};
	std::copy(stride.begin(), stride.end(), st);
	gcmxCheck(gcmx_snapshot_strided(ctx_, p.lo, p.hi, st, velocity ? 1 : 0, (int)quantities.size(), quantities.data(),
	                                velocity, values),
	          "gcmx_snapshot_strided");
}

template <int D>
std::vector<real> HipMesh<D>::gather(const NodeList& nodes, const std::vector<int>& quantities) const {
	std::vector<real> out(quantities.size() * nodes.size);
	gcmxCheck(gcmx_gather(ctx_, nodes.handle, (int)quantities.size(), quantities.data(), out.data()), "gcmx_gather");
	return out;
}

template <int D>
std::shared_ptr<typename HipMesh<D>::Recorder> HipMesh<D>::recorder(const std::vector<IntD>& nodes,
                                                                    const std::vector<int>& quantities,
                                                                    int capacity) const {
	const std::shared_ptr<NodeList> list = nodeList(nodes);  // copied by the recorder
	auto rec = std::make_shared<Recorder>();
	gcmxCheck(gcmx_recorder_create(ctx_, list->handle, (int)quantities.size(), quantities.data(), capacity, &rec->handle),
	          "gcmx_recorder_create");
	rec->receivers = nodes.size();
	rec->quantities = quantities.size();
	return rec;
}

template <int D>
std::shared_ptr<typename HipMesh<D>::Recorder> HipMesh<D>::recorder(const std::vector<std::array<real, D>>& points,
                                                                    const std::vector<int>& quantities,
                                                                    int capacity) const {
	std::vector<double> flat;
	flat.reserve(points.size() * D);
	for (const auto& pos : points) {
		// this mesh's inner nodes first (a stack member's neighbours are inner nodes
		// of the context too), then the place in the context
		IntD lo{}, hi{};
		for (int d = 0; d < D; d++) {
			if (!(pos[d] >= 0 && pos[d] <= (real)(this->sizes[d] - 1)))
				throw Exception("recorder: a point outside the inner nodes of the mesh");
			hi[d] = 1;
		}
		const PlacedBox p = placeBox(lo, hi, 0, "recorder: only inner nodes can be observed");
		for (int d = 0; d < D; d++) flat.push_back(pos[d] + (real)p.lo[d]);
	}
	auto rec = std::make_shared<Recorder>();
	gcmxCheck(gcmx_recorder_create_points(ctx_, (int)points.size(), flat.data(), (int)quantities.size(), quantities.data(),
	                                      capacity, &rec->handle),
	          "gcmx_recorder_create_points");
	rec->receivers = points.size();
	rec->quantities = quantities.size();
	return rec;
}

template <int D>
void HipMesh<D>::record(Recorder& rec) const {
	gcmxCheck(gcmx_record(ctx_, rec.handle), "gcmx_record");
}

template <int D>
std::vector<real> HipMesh<D>::readRecorder(Recorder& rec) const {
	const int count = rec.count();
	std::vector<real> out((size_t)count * rec.quantities * rec.receivers);
	if (count == 0) return out;
	gcmxCheck(gcmx_recorder_read(rec.handle, 0, count, out.data()), "gcmx_recorder_read");
	gcmxCheck(gcmx_recorder_reset(rec.handle), "gcmx_recorder_reset");
	return out;
}

template <int D>
std::array<uint64_t, 2> HipMesh<D>::transferBytes() const {
	uint64_t v[2] = {0, 0};
	gcmxCheck(gcmx_transfer_stats(ctx_, v), "gcmx_transfer_stats");
	return {v[0], v[1]};
}

// ----------------------------------------------------------------- the stage --

template <int D>
void HipGridCharacteristicMethod<D>::stage(const int s, const real& timeStep,
                                           AbstractGrid& mesh_) const {
	HipMesh<D>& mesh = dynamic_cast<HipMesh<D>&>(mesh_);  // std::bad_cast like the reference
	gcmxCheck(gcmx_stage(mesh.ctx(), s, timeStep), "gcmx_stage");
}

template <int D>
void HipGridCharacteristicMethod<D>::step(const real& timeStep, HipMesh<D>& mesh) const {
	gcmxCheck(gcmx_step(mesh.ctx(), timeStep), "gcmx_step");
}

// ------------------------------------------------------------ border conditions --

static int quantityCode(PhysicalQuantities::T q) { return static_cast<int>(q); }

template <int D>
HipBorderConditions<D>::HipBorderConditions(const Task& task, const HipMesh<D>& mesh) {
	const auto found = task.cubicBorderConditions.find(mesh.id);
	if (found == task.cubicBorderConditions.end()) {
		uniform = true;  // no face has a condition
		return;
	}
	// per face, per face node (forEachInner order): the last condition whose
	// area contains the node (later conditions overwrite the whole ghost)
	std::array<std::vector<int>, 6> effective;
	for (int f = 0; f < 2 * D; f++) {
		size_t n = 1;
		for (int d = 0; d < D; d++)
			if (d != f / 2) n *= (size_t)mesh.sizes[d];
		effective[f].assign(n, -1);
	}
	try {
		for (const auto& bc : found->second) {
			Condition c;
			c.direction = bc.direction;
			if (!(bc.direction >= 0 && bc.direction < D)) throw Exception("border direction out of range");
			for (const auto& q : bc.values) {
				if (!hasQuantityOf(mesh.model(), D, q.first)) throw Exception("border quantity not in the PDE vector");
				c.values.push_back({q.first, q.second});  // std::map order == reference order
			}
			if (c.values.size() > GCMX_MAX_BORDER_Q) throw Exception("too many border quantities");
			const int index = (int)conditions.size();
			auto collect = [&](int side, std::vector<int>& out) {
				std::vector<int>& eff = effective[2 * bc.direction + side];
				size_t k = 0;
				forEachInner<D>(mesh.sizes, [&](const std::array<int, D>& it) {
					if (bc.area->contains(mesh.coords(it))) {
						for (int d = 0; d < D; d++) out.push_back(it[d]);
						eff[k] = index;
					}
					k++;
				}, bc.direction, side ? mesh.sizes[bc.direction] - 1 : 0);
			};
			collect(0, c.leftNodes);
			collect(1, c.rightNodes);
			try {
				gcmxCheck(gcmx_border_nodes_create(mesh.ctx(), c.direction, -1, (int)(c.leftNodes.size() / D),
				                                   c.leftNodes.data(), &c.leftD), "gcmx_border_nodes_create");
				gcmxCheck(gcmx_border_nodes_create(mesh.ctx(), c.direction, +1, (int)(c.rightNodes.size() / D),
				                                   c.rightNodes.data(), &c.rightD), "gcmx_border_nodes_create");
			} catch (...) {
				gcmx_border_nodes_destroy(c.leftD);
				throw;
			}
			conditions.push_back(std::move(c));
		}
	} catch (...) {  // the destructor does not run for a constructor that throws
		for (auto& done : conditions) {
			gcmx_border_nodes_destroy(done.leftD);
			gcmx_border_nodes_destroy(done.rightD);
		}
		conditions.clear();
		throw;
	}
	uniform = true;
	for (int f = 0; f < 2 * D; f++) {
		const std::vector<int>& eff = effective[f];
		for (int e : eff) uniform = uniform && e == eff[0];
		faceCondition[f] = eff.empty() ? -1 : eff[0];
	}
	const char* noMaps = std::getenv("GCMX_NO_FACE_MAPS");  // 1: node lists only
	if (!uniform && conditions.size() <= GCMX_MAX_FACE_CONDITIONS && !(noMaps && std::atoi(noMaps) != 0)) {
		// partial faces: each face node's last condition, as one byte per face node
		std::array<std::vector<uint8_t>, 6> maps;
		const uint8_t* ptr[6] = {};
		for (int f = 0; f < 2 * D; f++) {
			maps[f].resize(effective[f].size());
			for (size_t k = 0; k < effective[f].size(); k++)
				maps[f][k] = effective[f][k] < 0 ? (uint8_t)GCMX_NO_FACE_CONDITION : (uint8_t)effective[f][k];
			ptr[f] = maps[f].data();
		}
		if (gcmx_face_map_create(mesh.ctx(), ptr, &faceMap_) != GCMX_OK) {
			// the map only lets the one-pass step take the partial faces: without
			// it the conditions' node lists (above) still serve every stage, so the
			// engine runs on the per-stage path
			std::fprintf(stderr, "gcm_amd: gcmx_face_map_create failed (%s); partial faces run on the per-stage path\n",
			             gcmx_last_error());
			faceMap_ = nullptr;
		}
	}
}

template <int D>
int HipBorderConditions<D>::conditionsAt(gcmx_face* out) const {
	for (size_t k = 0; k < conditions.size(); k++) {
		const Condition& c = conditions[k];
		out[k] = gcmx_face{};
		out[k].enabled = 1;
		out[k].n_quantities = (int)c.values.size();
		for (size_t i = 0; i < c.values.size(); i++) {
			out[k].quantities[i] = quantityCode(c.values[i].first);
			out[k].values[i] = c.values[i].second(Clock::Time());
		}
	}
	return (int)conditions.size();
}

template <int D>
HipBorderConditions<D>::~HipBorderConditions() {
	gcmx_face_map_destroy(faceMap_);
	for (auto& c : conditions) {
		gcmx_border_nodes_destroy(c.leftD);
		gcmx_border_nodes_destroy(c.rightD);
	}
}

template <int D>
void HipBorderConditions<D>::apply(AbstractGrid& mesh_, const int direction) const {
	HipMesh<D>& mesh = dynamic_cast<HipMesh<D>&>(mesh_);
	for (const auto& c : conditions) {
		if (c.direction != direction) continue;
		std::vector<int> qs;
		std::vector<real> vals;
		for (const auto& v : c.values) {
			qs.push_back(quantityCode(v.first));
			vals.push_back(v.second(Clock::Time()));
		}
		gcmxCheck(gcmx_border_apply(mesh.ctx(), c.leftD, (int)qs.size(), qs.data(), vals.data()),
		          "gcmx_border_apply");
		gcmxCheck(gcmx_border_apply(mesh.ctx(), c.rightD, (int)qs.size(), qs.data(), vals.data()),
		          "gcmx_border_apply");
	}
}

template <int D>
void HipBorderConditions<D>::faces(gcmx_face* out) const {
	for (int f = 0; f < 2 * D; f++) {
		out[f] = gcmx_face{};
		if (faceCondition[f] < 0) continue;
		const Condition& c = conditions[(size_t)faceCondition[f]];
		out[f].enabled = 1;
		out[f].n_quantities = (int)c.values.size();
		for (size_t k = 0; k < c.values.size(); k++) {
			out[f].quantities[k] = quantityCode(c.values[k].first);
			out[f].values[k] = c.values[k].second(Clock::Time());
		}
	}
}

template <int D>
void HipContactCopier<D>::apply(HipMesh<D>& a, const HipMesh<D>& b) const {
	gcmxCheck(gcmx_copy_box(a.ctx(), dmin.data(), dmax.data(), b.ctx(), smin.data()), "gcmx_copy_box");
}

// --------------------------------------------------------------------- Engine --

template <int D>
Engine<D>::Engine(const Task& task, int device_)
    : AbstractEngine(task), device(device_), stateChunkBytes(task.vtkSnapshotter.chunkBytes) {
	if (task.globalSettings.dimensionality != D) throw Exception("dimensionality mismatch");
	createGridsAndContacts(task);
	buildStacks(task);
	std::map<size_t, SetUpLists<D>> memberLists;  // of the bodies in stacks
	for (const auto& tb : task.bodies) {
		Body& body = getBody(tb.first);
		if (body.stack) memberLists.emplace(tb.first, dynamic_cast<HipMesh<D>&>(*body.mesh).setUpMember(task));
		else body.mesh->setUpPde(task);
		body.gcm = body.factory->createGcm(task);
		body.border = body.factory->createBorder(task, body.mesh);
		for (const Snapshotters::T snapType : task.globalSettings.snapshottersId)
			body.snapshotters.push_back(body.factory->createSnapshotter(task, snapType));
		for (const Odes::T odeType : tb.second.odes) body.odes.push_back(body.factory->createOde(odeType));
	}
	for (Body& lead : bodies) {  // every stack's set-up from its members' lists
		if (!lead.stackLead) continue;
		std::vector<HipMesh<D>*> members;
		std::vector<SetUpLists<D>> lists;
		for (size_t id : stackOrder_.at(lead.mesh->id)) {
			members.push_back(&dynamic_cast<HipMesh<D>&>(*getBody(id).mesh));
			lists.push_back(std::move(memberLists.at(id)));
		}
		lead.stack->setUp(members, lists, task.cubicGrid.setUpOnDevice);
	}
	afterConstruction(task);
}

template <int D>
typename Engine<D>::Body& Engine<D>::getBody(size_t id) {
	for (Body& b : bodies)
		if (b.mesh->id == id) return b;
	throw Exception("There isn't a body with given id");
}

template <int D>
const typename Engine<D>::Body& Engine<D>::getBody(size_t id) const {
	for (const Body& b : bodies)
		if (b.mesh->id == id) return b;
	throw Exception("There isn't a body with given id");
}

template <int D>
std::shared_ptr<const HipMesh<D>> Engine<D>::getMesh(size_t gridId) const {
	return std::dynamic_pointer_cast<const HipMesh<D>>(getBody(gridId).mesh);
}

// Engine.cpp:38-87 (factory choice: Engine.cpp:155-189)
template <int D>
void Engine<D>::createGridsAndContacts(const Task& task) {
	if (task.bodies.empty()) throw Exception("the task has no bodies");
	if (task.bodies.size() != task.cubicGrid.cubics.size())
		throw Exception("every body needs a cube");
	// The three products of Engine<D>::createAbstractFactory (Engine.cpp:155-189):
	// ISOTROPIC x ELASTIC, ORTHOTROPIC x ELASTIC, ISOTROPIC x ACOUSTIC.  An
	// acoustic body stands alone (contacts and stacks are elastic-only here) and
	// has no ODE (AcousticModel::OdeVariables is void).
	size_t nAcoustic = 0;
	for (const auto& tb : task.bodies) nAcoustic += tb.second.modelId == Models::T::ACOUSTIC;
	if (nAcoustic > 0 && nAcoustic < task.bodies.size()) throw Exception("a task must not mix acoustic and elastic bodies");
	if (nAcoustic > 1) throw Exception("at most one acoustic body (contacts between acoustic bodies are not implemented)");
	for (const auto& tb : task.bodies) {
		if (tb.second.modelId != Models::T::ELASTIC && tb.second.modelId != Models::T::ACOUSTIC)
			throw Exception("unknown model");
		if (tb.second.modelId == Models::T::ACOUSTIC) {
			if (tb.second.materialId != Materials::T::ISOTROPIC)
				throw Exception("ORTHOTROPIC x ACOUSTIC is not a product of the cubic engine");
			if (!tb.second.odes.empty()) throw Exception("the acoustic model has no ODE");
		}
		if (tb.second.materialId == Materials::T::ORTHOTROPIC && D != 3)
			throw Exception("orthotropic media are implemented in 3-D only");
		Body body;
		body.factory = std::make_shared<HipFactory<D>>(device);
		const auto cp = constructionPack<D>(task, tb.first);
		body.mesh = body.factory->createMesh(task, tb.first, cp, 1);
		bodies.push_back(body);
	}
	for (Body& body : bodies) {
		for (const Body& other : bodies) {
			if (other.mesh->id == body.mesh->id) continue;
			auto a = body.mesh->aabb(), b = other.mesh->aabb();
			std::array<int, D> mn, mx, w;
			bool valid = true;
			for (int i = 0; i < D; i++) {
				mn[i] = std::max(a.first[i], b.first[i]);
				mx[i] = std::min(a.second[i], b.second[i]);
				w[i] = mx[i] - mn[i];
				if (w[i] < 0) valid = false;
			}
			if (valid) throw Exception("Bodies must not intersect");
			int axis = 0;
			int minW = w[0];
			for (int i = 1; i < D; i++)
				if (w[i] < minW) {
					axis = i;
					minW = w[i];
				}
			if (minW != -1) continue;  // no contact
			std::array<int, D> bmin = mn, bmax = mx;
			if (body.mesh->start[axis] > other.mesh->start[axis]) bmin[axis] -= body.mesh->borderSize;
			else bmax[axis] += body.mesh->borderSize;
			std::array<int, 3> dmin{0, 0, 0}, dmax{1, 1, 1}, smin{0, 0, 0};
			for (int i = 0; i < D; i++) {
				dmin[i] = bmin[i] - body.mesh->start[i];
				dmax[i] = bmax[i] - body.mesh->start[i] + 1;
				smin[i] = bmin[i] - other.mesh->start[i];
			}
			typename Body::Contact contact;
			contact.neighborId = other.mesh->id;
			contact.direction = axis;
			contact.copier = std::make_shared<HipContactCopier<D>>(dmin, dmax, smin);
			body.contacts.push_back(contact);
		}
	}
}

// Stacks (HipMesh::joinStack): chains of 3-D bodies along one axis whose every
// contact lies along that axis, between bodies of equal sizes and starts on the
// other two axes, with no border conditions and the same ODEs.  Their contact
// copies then only ever write what the stack's own stages read, so the chain
// runs as one grid: one launch of the one-pass step over all its nodes (along
// x the separate bodies could take the one-pass step too, but each as a thin
// launch with short y chunks, plus the contact copies: 256^3 as 4 x-bodies
// 0.86 ms/step against 0.57 as one grid).  The inner nodes are the separate
// bodies' bitwise; ghost layers at a contact hold the neighbour's current inner
// nodes instead of the copy made before the last stage (scratch: no output
// reads them).  GCMX_NO_STACKS=1 keeps the separate bodies (A/B, tests).
template <int D>
void Engine<D>::buildStacks(const Task& task) {
	if (D != 3) return;
	if (const char* e = std::getenv("GCMX_NO_STACKS"))
		if (std::atoi(e) != 0) return;
	auto hasBorder = [&](size_t id) {
		const auto f = task.cubicBorderConditions.find(id);
		return f != task.cubicBorderConditions.end() && !f->second.empty();
	};
	for (int a = 0; a < D; a++) {
		std::map<size_t, bool> ok;  // every contact along a, partners of equal cross-section
		for (Body& b : bodies) {
			bool good = !b.stack && !b.contacts.empty() && !hasBorder(b.mesh->id);
			for (const auto& c : b.contacts) {
				if (c.direction != a) good = false;
				const Body& o = getBody(c.neighborId);
				for (int d = 0; d < D; d++)
					if (d != a && (o.mesh->sizes[d] != b.mesh->sizes[d] || o.mesh->start[d] != b.mesh->start[d]))
						good = false;
			}
			ok[b.mesh->id] = good;
		}
		std::map<size_t, bool> seen;
		for (Body& b : bodies) {
			const size_t id0 = b.mesh->id;
			if (!ok[id0] || seen[id0]) continue;
			std::vector<size_t> comp, todo{id0};
			seen[id0] = true;
			bool allGood = true;
			while (!todo.empty()) {  // the bodies connected to id0 by contacts
				const size_t id = todo.back();
				todo.pop_back();
				comp.push_back(id);
				for (const auto& c : getBody(id).contacts) {
					if (!ok[c.neighborId]) allGood = false;
					if (!seen[c.neighborId]) {
						seen[c.neighborId] = true;
						todo.push_back(c.neighborId);
					}
				}
			}
			if (!allGood || comp.size() < 2) continue;
			std::sort(comp.begin(), comp.end(),
			          [&](size_t p, size_t q) { return getBody(p).mesh->start[a] < getBody(q).mesh->start[a]; });
			bool chain = true;
			int total = 0;
			for (size_t k = 0; k < comp.size(); k++) {
				const auto& m = *getBody(comp[k]).mesh;
				if (k > 0) {
					const auto& p = *getBody(comp[k - 1]).mesh;
					chain = chain && m.start[a] == p.start[a] + p.sizes[a];
					chain = chain && task.bodies.at(comp[k]).odes == task.bodies.at(comp[0]).odes;
				}
				total += m.sizes[a];
			}
			if (!chain) continue;
			auto cp = constructionPack<D>(task, comp[0]);
			cp.sizes[a] = total;
			auto stack = std::make_shared<HipMesh<D>>(task, comp[0], cp, device);
			int off = 0;
			for (size_t id : comp) {
				Body& m = getBody(id);
				auto hm = std::dynamic_pointer_cast<HipMesh<D>>(m.mesh);
				hm->joinStack(stack, a, off);
				off += hm->sizes[a];
				m.stack = stack;
				m.contacts.clear();  // inside the stack: its own rows
			}
			getBody(comp[0]).stackLead = true;
			stackOrder_[comp[0]] = comp;
		}
	}
}

template <int D>
HipMesh<D>* Engine<D>::unitMesh(Body& b) {
	if (b.stack) return b.stackLead ? b.stack.get() : nullptr;
	return &dynamic_cast<HipMesh<D>&>(*b.mesh);
}

// Engine.cpp:90-121
template <int D>
void Engine<D>::nextTimeStep() {
	bool plain = true, faces = true, xcontacts = D == 3;
	for (const Body& b : bodies) {
		plain = plain && b.border->empty() && b.contacts.empty();
		faces = faces && (b.border->uniformFaces() || b.border->faceMap()) && b.contacts.empty();
		xcontacts = xcontacts && b.border->empty();
		for (const auto& contact : b.contacts) xcontacts = xcontacts && contact.direction == 0;
	}
	// A body whose only ODE is MaxwellViscosityOde hands it to the library with
	// the step (gcmx_step_ode): the same results as the stages followed by the ODE
	// (Engine.cpp:115-119), in one pass over the layer where the step is fused.
	auto oneMaxwell = [](const Body& b) {
		return b.odes.size() == 1 && dynamic_cast<const HipMaxwellViscosityOde<D>*>(b.odes[0].get()) != nullptr;
	};
	if (plain || xcontacts) {
		// No border or contact work between the stages: one gcmx_step per body
		// (identical results; lets the library use its fused kernels).  3-D
		// bodies whose contacts all lie along x: every ContactCopier of the step
		// runs before stage 0 and reads the neighbours' layer E_n
		// (Engine.cpp:99-107), and only stage 0 reads x ghosts, so all copies go
		// first, then one gcmx_step per body (the x-ghost copy keeps the
		// one-pass step admissible, gcmx_copy_box).
		if (!plain)
			for (Body& body : bodies)
				for (auto& contact : body.contacts)
					contact.copier->apply(dynamic_cast<HipMesh<D>&>(*body.mesh),
					                      dynamic_cast<const HipMesh<D>&>(*getBody(contact.neighborId).mesh));
		for (Body& b : bodies) {
			HipMesh<D>* um = unitMesh(b);
			if (!um) continue;  // a stack member stepped by its lead
			HipMesh<D>& mesh = *um;
			if (oneMaxwell(b)) {
				const auto& tau0 = mesh.deviceTau0();
				gcmxCheck(gcmx_step_ode(mesh.ctx(), Clock::TimeStep(), nullptr, tau0.data(), (int)tau0.size()),
				          "gcmx_step_ode");
				continue;
			}
			std::static_pointer_cast<HipGridCharacteristicMethod<D>>(b.gcm)->step(Clock::TimeStep(), mesh);
			for (auto& ode : b.odes) ode->apply(mesh, Clock::TimeStep());
		}
		return;
	}
	if (faces) {
		// Whole-face border conditions and no contacts: every stage's
		// BorderConditions::apply is a function of the face only, so the library
		// runs the step (fused where admissible) with the faces' values at
		// Clock::Time() -- the time all D stages of the reference step see.
		for (Body& b : bodies) {
			HipMesh<D>* um = unitMesh(b);
			if (!um) continue;
			HipMesh<D>& mesh = *um;
			if (const gcmx_face_map* fm = b.border->faceMap()) {
				// partial faces: each face node's own last condition, the whole step in
				// the library (one pass where admissible), then the ODEs
				gcmx_face conds[GCMX_MAX_FACE_CONDITIONS];
				const int n = b.border->conditionsAt(conds);
				gcmxCheck(gcmx_step_face_map(mesh.ctx(), Clock::TimeStep(), fm, n, conds), "gcmx_step_face_map");
				for (auto& ode : b.odes) ode->apply(mesh, Clock::TimeStep());
				continue;
			}
			gcmx_face f[6];
			b.border->faces(f);
			if (oneMaxwell(b)) {
				const auto& tau0 = mesh.deviceTau0();
				gcmxCheck(gcmx_step_ode(mesh.ctx(), Clock::TimeStep(), f, tau0.data(), (int)tau0.size()),
				          "gcmx_step_ode");
				continue;
			}
			gcmxCheck(gcmx_step_faces(mesh.ctx(), Clock::TimeStep(), f), "gcmx_step_faces");
			for (auto& ode : b.odes) ode->apply(mesh, Clock::TimeStep());
		}
		return;
	}
	for (int stage = 0; stage < D; stage++) {
		for (Body& body : bodies) body.border->apply(*body.mesh, stage);
		for (Body& body : bodies)
			for (auto& contact : body.contacts)
				if (contact.direction == stage)
					contact.copier->apply(dynamic_cast<HipMesh<D>&>(*body.mesh),
					                      dynamic_cast<const HipMesh<D>&>(*getBody(contact.neighborId).mesh));
		for (Body& body : bodies) {
			HipMesh<D>* um = unitMesh(body);
			if (!um) continue;
			body.gcm->stage(stage, Clock::TimeStep(), *um);
			um->swapCurrAndNextPdeTimeLayer(0);
		}
	}
	applyOdes();
}

// Engine.cpp:115-119: ODEs after all stages of the step.
template <int D>
void Engine<D>::applyOdes() {
	for (Body& body : bodies) {
		HipMesh<D>* um = unitMesh(body);
		if (!um) continue;
		for (auto& ode : body.odes) ode->apply(*um, Clock::TimeStep());
	}
}

template <int D>
void Engine<D>::writeSnapshots(const int step) {
	for (Body& body : bodies)
		for (auto& snap : body.snapshotters) snap->snapshot(body.mesh.get(), step);
}

template <int D>
void Engine<D>::flushSnapshots() const {
	for (const Body& body : bodies)
		for (auto& snap : body.snapshotters) snap->flush();
}

template <int D>
Engine<D>::~Engine() {
	try {
		flushSnapshots();
	} catch (...) {  // a destructor: what could not be written is lost
	}
}

// ------------------------------------------------------------ save and resume --

template <int D>
StateFileHeader Engine<D>::stateHeader() const {
	StateFileHeader h;
	h.D = D;
	h.steps = steps;
	h.time = Clock::Time();
	h.timeStep = Clock::TimeStep();
	for (const Body& body : bodies) {
		const HipMesh<D>& mesh = dynamic_cast<const HipMesh<D>&>(*body.mesh);
		StateFileBody b;
		b.id = mesh.id;
		b.model = mesh.model();
		b.M = (uint32_t)mesh.pdeM();
		for (int d = 0; d < D; d++) b.sizes[d] = (uint32_t)mesh.sizes[d];
		h.bodies.push_back(b);
	}
	return h;
}

namespace {

// Slabs along x of the inner nodes of `sizes`: at most chunkBytes each, one x
// plane at least.  f(lo, hi, bytes of the slab).
template <int D, typename F>
void forEachStateSlab(const std::array<int, D>& sizes, int M, size_t chunkBytes, F f) {
	size_t plane = (size_t)M * sizeof(real);
	for (int d = 1; d < D; d++) plane *= (size_t)sizes[d];
	const int thick = (int)std::min<size_t>((size_t)sizes[0], std::max<size_t>(1, chunkBytes / plane));
	for (int x0 = 0; x0 < sizes[0]; x0 += thick) {
		std::array<int, D> lo{}, hi = sizes;
		lo[0] = x0;
		hi[0] = std::min(x0 + thick, sizes[0]);
		f(lo, hi, (size_t)(hi[0] - x0) * plane);
	}
}

}  // namespace

template <int D>
void Engine<D>::saveState(const std::string& path) const {
	flushSnapshots();  // the files of the saved run are complete up to the saved step
	const StateFileHeader h = stateHeader();
	StateFileWriter w(path);
	w.writeHeader(h);
	std::vector<real> slab;  // one slab, never a layer
	for (size_t k = 0; k < bodies.size(); k++) {
		const HipMesh<D>& mesh = dynamic_cast<const HipMesh<D>&>(*bodies[k].mesh);
		w.writeBodyRecord(h.bodies[k]);
		forEachStateSlab<D>(mesh.sizes, mesh.pdeM(), stateChunkBytes, [&](const auto& lo, const auto& hi, size_t bytes) {
			slab.resize(bytes / sizeof(real));
			mesh.readBox(lo, hi, slab.data(), stateChunkBytes);
			w.write(slab.data(), bytes);
		});
	}
	if (w.written() != stateFileOffsets(h).back()) throw Exception("saveState: wrote another size than the header says");
	w.commit();
}

template <int D>
void Engine<D>::loadState(const std::string& path) {
	// everything that can be refused, before the first node changes
	const StateFileHeader file = readStateFileHeader(path);
	checkStateFileHeader(file, stateHeader());
	const std::vector<uint64_t> offsets = stateFileOffsets(file);
	std::FILE* f = std::fopen(path.c_str(), "rb");
	if (!f) throw Exception("state file " + path + ": cannot open");
	struct Close {
		std::FILE* f;
		~Close() { std::fclose(f); }
	} closer{f};
	std::vector<real> slab;
	for (size_t k = 0; k < bodies.size(); k++) {
		HipMesh<D>& mesh = dynamic_cast<HipMesh<D>&>(*bodies[k].mesh);
		if (std::fseek(f, (long)offsets[k], SEEK_SET) != 0) throw Exception("state file " + path + ": cannot seek");
		forEachStateSlab<D>(mesh.sizes, mesh.pdeM(), stateChunkBytes, [&](const auto& lo, const auto& hi, size_t bytes) {
			slab.resize(bytes / sizeof(real));
			if (std::fread(slab.data(), 1, bytes, f) != bytes) throw Exception("state file " + path + ": read failed");
			mesh.writeBox(lo, hi, slab.data(), stateChunkBytes);
		});
	}
	restoreClock((int)file.steps, file.time, file.timeStep);
}

// ------------------------------------------------------------- snapshotters --

template <int D>
void VtkSnapshotter<D>::snapshotImpl(const AbstractGrid* mesh_, const int step) {
	const HipMesh<D>* mesh = dynamic_cast<const HipMesh<D>*>(mesh_);
	if (!mesh) throw Exception("VtkSnapshotter: not a cubic mesh");
	VtkSelection<D> sel;
	if (!vtkSelectionOf<D>(settings, mesh->sizes, mesh->start, sel)) return;  // the box misses this body
	const size_t n = sel.points();
	VtsArray vel{"Velocity", 3, std::vector<float>(3 * n)};
	std::vector<VtsArray> qs;
	std::vector<int> codes;
	for (auto q : quantitiesToSnap) {
		if (!hasQuantityOf(mesh->model(), D, q)) throw Exception("quantity to snap is not in this PDE vector");
		qs.push_back(VtsArray{quantityName(q), 1, std::vector<float>(n)});
		codes.push_back(quantityCode(q));
	}
	// Slabs along the slowest VTK axis (the last one), counted in output indices:
	// whole lines and planes of the file's point order, so a slab's arrays are
	// contiguous parts of the file's.
	const int slow = D - 1;
	const size_t nSlow = (size_t)sel.points(slow);
	const size_t plane = n / nSlow;  // points per index of the slow axis
	const size_t perPoint = 4 * (3 + qs.size());
	const size_t thick = std::max<size_t>(1, chunkBytes / (plane * perPoint));
	std::vector<float> slab;  // [quantities][points of the slab], when there are several
	for (size_t s0 = 0; s0 < nSlow; s0 += thick) {
		const size_t s1 = std::min<size_t>(s0 + thick, nSlow);
		std::array<int, D> lo = sel.lo, hi = sel.hi;
		lo[slow] = sel.lo[slow] + (int)s0 * sel.stride[slow];
		hi[slow] = std::min(sel.hi[slow], sel.lo[slow] + (int)(s1 - 1) * sel.stride[slow] + 1);
		const size_t first = s0 * plane, count = (s1 - s0) * plane;
		float* values = nullptr;
		if (qs.size() == 1) values = qs[0].values.data() + first;
		if (qs.size() > 1) {
			slab.resize(qs.size() * count);
			values = slab.data();
		}
		mesh->snapshotArrays(lo, hi, sel.stride, codes, vel.values.data() + 3 * first, values);
		if (qs.size() > 1)
			for (size_t k = 0; k < qs.size(); k++)
				std::copy(slab.begin() + k * count, slab.begin() + (k + 1) * count, qs[k].values.begin() + first);
	}
	const auto& ids = mesh->materialIdsAll();
	writeVtkArrays<D>(makeFileNameForSnapshot(std::to_string(mesh->id), step, "vts", "vtk"), mesh->sizes,
	                  mesh->start, mesh->h, mesh->borderSize, ids.empty() ? nullptr : ids.data(),
	                  mesh->materialNumbers(), sel, std::move(vel), std::move(qs));
}

template <int D>
SliceSnapshotter<D>::SliceSnapshotter(const Task& task) : Snapshotter(task) {
	if (task.detector.quantities.size() != 1)  // SliceSnapshotter.hpp:31
		throw Exception("SliceSnapshotter: exactly one detector quantity is supported");
	quantityToWrite = task.detector.quantities[0];
	detectionArea = task.detector.area;
	gridId = task.detector.gridId;
	if (!detectionArea) throw Exception("SliceSnapshotter: detector area missing");
	bufferSteps = task.detector.bufferSteps;
	if (bufferSteps < 0) throw Exception("SliceSnapshotter: detector.bufferSteps is at least 0");
}

template <int D>
void SliceSnapshotter<D>::snapshotImpl(const AbstractGrid* mesh_, const int step) {
	const HipMesh<D>* mesh = dynamic_cast<const HipMesh<D>*>(mesh_);
	if (!mesh) throw Exception("SliceSnapshotter: not a cubic mesh");
	const int direction = D - 1;
	if (listsOf != mesh) {  // first use: the node lists go to the device once
		column.reset();
		detector.reset();
		listsOf = mesh;
		// along the last axis through sizes / 2 (SliceSnapshotter.hpp:45-63)
		std::array<int, D> it;
		for (int i = 0; i < D; i++) it[i] = mesh->sizes[i] / 2;
		std::vector<std::array<int, D>> nodes;
		for (int k = 0; k < mesh->sizes[direction]; k++) {
			it[direction] = k;
			nodes.push_back(it);
		}
		const int VzCode = quantityCode(PhysicalQuantities::T::Vx) + direction;
		if (bufferSteps > 0) columnRec = mesh->recorder(nodes, {VzCode}, bufferSteps);
		else column = mesh->nodeList(nodes);
		if (mesh->id == gridId) {
			// upper detector: the right border of the last axis inside the area (hpp:65-88)
			if (!hasQuantityOf(mesh->model(), D, quantityToWrite)) throw Exception("quantity not present in the PDE vector");
			nodes.clear();
			forEachInner<D>(mesh->sizes, [&](const std::array<int, D>& j) {
				if (j[direction] != mesh->sizes[direction] - 1) return;
				if (detectionArea->contains(mesh->coords(j))) nodes.push_back(j);
			});
			if (nodes.empty()) throw Exception("SliceSnapshotter: no node in the detection area");
			if (bufferSteps > 0) detectorRec = mesh->recorder(nodes, {quantityCode(quantityToWrite)}, bufferSteps);
			else detector = mesh->nodeList(nodes);
		}
	}
	if (bufferSteps > 0) {
		// the sample stays on the device: no wait here, the files at the next flush
		mesh->record(*columnRec);
		if (detectorRec) mesh->record(*detectorRec);
		heldSteps.push_back(step);
		heldTimes.push_back(Clock::Time());
		if ((int)heldSteps.size() == bufferSteps) flush();
		return;
	}
	const std::vector<real> Vz = mesh->gather(*column, {quantityCode(PhysicalQuantities::T::Vx) + direction});
	std::vector<real> valuesInArea;
	if (mesh->id == gridId) valuesInArea = mesh->gather(*detector, {quantityCode(quantityToWrite)});
	writeFiles(mesh, step, Clock::Time(), Vz.data(), valuesInArea.data(), valuesInArea.size());
}

// The files of one snapshot from its column and, on body gridId, its detector values.
template <int D>
void SliceSnapshotter<D>::writeFiles(const HipMesh<D>* mesh, int step, real time, const real* Vz_,
                                     const real* valuesInArea, size_t nValues) {
	const int direction = D - 1;
	std::array<int, D> it;
	for (int i = 0; i < D; i++) it[i] = mesh->sizes[i] / 2;
	std::vector<real> coordZ;
	for (int k = 0; k < mesh->sizes[direction]; k++) {
		it[direction] = k;
		coordZ.push_back(mesh->coords(it)[direction]);
	}
	const std::vector<real> Vz(Vz_, Vz_ + coordZ.size());
	writeColumns(makeFileNameForSnapshot(std::to_string(mesh->id), step, "txt", "zaxis"),
	             {coordZ, Vz});
	if (mesh->id != gridId) return;
	real sum = 0;
	for (size_t i = 0; i < nValues; i++) sum += valuesInArea[i];  // std::accumulate order
	const real valueToWrite = sum / (real)nValues;
	times.push_back(time);
	seismo.push_back((precision)valueToWrite);
	writeColumns(makeFileNameForSnapshot(std::to_string(mesh->id), step, "txt", "detector"),
	             {times, seismo});
}

template <int D>
void SliceSnapshotter<D>::flush() {
	if (heldSteps.empty()) return;
	const HipMesh<D>* mesh = listsOf;
	const std::vector<real> Vz = mesh->readRecorder(*columnRec);
	std::vector<real> inArea;
	if (detectorRec) inArea = mesh->readRecorder(*detectorRec);
	const std::vector<int> stepsHeld = std::move(heldSteps);
	const std::vector<real> timesHeld = std::move(heldTimes);
	heldSteps.clear();
	heldTimes.clear();
	const size_t nColumn = columnRec->receivers, nArea = detectorRec ? detectorRec->receivers : 0;
	for (size_t s = 0; s < stepsHeld.size(); s++)
		writeFiles(mesh, stepsHeld[s], timesHeld[s], Vz.data() + s * nColumn, inArea.data() + s * nArea, nArea);
}

template <int D>
ReceiverSnapshotter<D>::ReceiverSnapshotter(const Task& task) : Snapshotter(task), settings(task.receivers) {
	if (settings.points.empty()) throw Exception("ReceiverSnapshotter: no receivers (Task::Receivers::points)");
	if (settings.quantities.empty() || settings.quantities.size() > GCMX_MAX_BORDER_Q)
		throw Exception("ReceiverSnapshotter: 1 to 16 quantities");
	if (settings.bufferSteps < 1) throw Exception("ReceiverSnapshotter: bufferSteps is at least 1");
}

template <int D>
void ReceiverSnapshotter<D>::snapshotImpl(const AbstractGrid* mesh_, const int step) {
	const HipMesh<D>* m = dynamic_cast<const HipMesh<D>*>(mesh_);
	if (!m) throw Exception("ReceiverSnapshotter: not a cubic mesh");
	if (m->id != settings.gridId) return;
	if (mesh != m) {  // first use: the receivers go to the device once
		std::vector<int> codes;
		for (auto q : settings.quantities) {
			if (!hasQuantityOf(m->model(), D, q)) throw Exception("quantity not present in the PDE vector");
			codes.push_back(quantityCode(q));
		}
		std::array<int, D> first{};
		const auto origin = m->coords(first);
		std::vector<std::array<real, D>> positions;
		for (const Real3& p : settings.points) {
			std::array<real, D> pos;
			for (int d = 0; d < D; d++) pos[d] = (p[d] - origin[d]) / m->h[d];
			positions.push_back(pos);
		}
		rec = m->recorder(positions, codes, settings.bufferSteps);  // throws for a point outside the body
		mesh = m;
	}
	m->record(*rec);
	heldSteps.push_back(step);
	heldTimes.push_back(Clock::Time());
	if ((int)heldSteps.size() == settings.bufferSteps) flush();
}

template <int D>
void ReceiverSnapshotter<D>::flush() {
	if (heldSteps.empty()) return;
	const std::vector<real> values = mesh->readRecorder(*rec);
	const std::vector<real> timesHeld = std::move(heldTimes);
	const int firstStep = heldSteps.front();
	const size_t rows = heldSteps.size(), row = rec->quantities * rec->receivers;
	heldSteps.clear();
	heldTimes.clear();
	const std::string fileName = makeFileNameForSnapshot(std::to_string(mesh->id), firstStep, "txt", "receivers");
	std::FILE* f = std::fopen(fileName.c_str(), "w");
	if (!f) throw Exception("cannot open " + fileName);
	bool ok = true;
	for (size_t s = 0; s < rows; s++) {
		ok = ok && std::fprintf(f, "%.17g", timesHeld[s]) > 0;
		for (size_t i = 0; i < row; i++) ok = ok && std::fprintf(f, "\t%.17g", values[s * row + i]) > 0;
		ok = ok && std::fputc('\n', f) != EOF;
	}
	ok = std::fclose(f) == 0 && ok;
	if (!ok) throw Exception("write failed: " + fileName);
}

template <int D>
void HipMaxwellViscosityOde<D>::apply(AbstractGrid& mesh_, const real timeStep) {
	HipMesh<D>& mesh = dynamic_cast<HipMesh<D>&>(mesh_);
	const auto& tau0 = mesh.deviceTau0();
	gcmxCheck(gcmx_ode_maxwell(mesh.ctx(), timeStep, tau0.data(), (int)tau0.size()),
	          "gcmx_ode_maxwell");
}

// Engine.cpp:124-140
template <int D>
real Engine<D>::estimateTimeStep() {
	real maxEigenvalue = 0;
	const auto h = bodies.front().mesh->h;
	for (const Body& b : bodies) {
		if (!(h == b.mesh->h)) throw Exception("all bodies must share h");
		const real e = b.mesh->getMaximalEigenvalue();
		if (e > maxEigenvalue) maxEigenvalue = e;
	}
	return CourantNumber * bodies.front().mesh->getMinimalSpatialStep() / maxEigenvalue;
}

template class CubicGrid<1>;
template class CubicGrid<2>;
template class CubicGrid<3>;
template class HipMesh<1>;
template class HipMesh<2>;
template class HipMesh<3>;
template class HipGridCharacteristicMethod<1>;
template class HipGridCharacteristicMethod<2>;
template class HipGridCharacteristicMethod<3>;
template class HipBorderConditions<1>;
template class HipBorderConditions<2>;
template class HipBorderConditions<3>;
template class HipContactCopier<1>;
template class HipContactCopier<2>;
template class HipContactCopier<3>;
template class VtkSnapshotter<1>;
template class VtkSnapshotter<2>;
template class VtkSnapshotter<3>;
template class SliceSnapshotter<1>;
template class SliceSnapshotter<2>;
template class SliceSnapshotter<3>;
template class ReceiverSnapshotter<1>;
template class ReceiverSnapshotter<2>;
template class ReceiverSnapshotter<3>;
template class HipMaxwellViscosityOde<1>;
template class HipMaxwellViscosityOde<2>;
template class HipMaxwellViscosityOde<3>;
template CubicGrid<1>::ConstructionPack constructionPack<1>(const Task&, size_t);
template CubicGrid<2>::ConstructionPack constructionPack<2>(const Task&, size_t);
template CubicGrid<3>::ConstructionPack constructionPack<3>(const Task&, size_t);
template HostState<1> buildHostState<1>(const Task&, const CubicGrid<1>&);
template HostState<2> buildHostState<2>(const Task&, const CubicGrid<2>&);
template HostState<3> buildHostState<3>(const Task&, const CubicGrid<3>&);
template SetUpLists<1> buildSetUpLists<1>(const Task&, const CubicGrid<1>&);
template SetUpLists<2> buildSetUpLists<2>(const Task&, const CubicGrid<2>&);
template SetUpLists<3> buildSetUpLists<3>(const Task&, const CubicGrid<3>&);
template void applySetUpLists<1>(const SetUpLists<1>&, const CubicGrid<1>&, std::vector<uint8_t>&, const CubicGrid<1>&,
                                  const std::array<int, 1>&, std::vector<real>&);
template void applySetUpLists<2>(const SetUpLists<2>&, const CubicGrid<2>&, std::vector<uint8_t>&, const CubicGrid<2>&,
                                  const std::array<int, 2>&, std::vector<real>&);
template void applySetUpLists<3>(const SetUpLists<3>&, const CubicGrid<3>&, std::vector<uint8_t>&, const CubicGrid<3>&,
                                  const std::array<int, 3>&, std::vector<real>&);
template MaterialTable<1> buildMaterialTable<1>(const std::vector<SetUpLists<1>>&, bool);
template MaterialTable<2> buildMaterialTable<2>(const std::vector<SetUpLists<2>>&, bool);
template MaterialTable<3> buildMaterialTable<3>(const std::vector<SetUpLists<3>>&, bool);
template class Engine<1>;
template class Engine<2>;
template class Engine<3>;

}  // namespace cubic

// engine/EngineFactory.hpp:11-38
std::shared_ptr<AbstractEngine> createEngine(const Task& task, int device) {
	if (task.globalSettings.gridId != Grids::T::CUBIC)
		throw Exception("only the cubic engine is on this path");
	switch (task.globalSettings.dimensionality) {
	case 1: return std::make_shared<cubic::Engine<1>>(task, device);
	case 2: return std::make_shared<cubic::Engine<2>>(task, device);
	case 3: return std::make_shared<cubic::Engine<3>>(task, device);
	default: throw Exception("Invalid dimensionality");
	}
}

}  // namespace gcm
