// engine.hpp -- host mirror of libgcm's cubic engine surface over the gcmx C-ABI.
//
// Same class roles and call order as the reference:
//   AbstractEngine (engine/AbstractEngine.{hpp,cpp})        -> gcm::AbstractEngine
//   Clock (engine/GlobalVariables.hpp:16-41)                 -> gcm::Clock
//   cubic::Engine<D> (engine/cubic/Engine.{hpp,cpp})         -> gcm::cubic::Engine<D>
//   cubic::AbstractFactoryBase / AbstractFactory             -> cubic::AbstractFactoryBase / HipFactory
//   cubic::AbstractMesh / DefaultMesh                        -> cubic::AbstractMesh / HipMesh
//   cubic::GridCharacteristicMethodBase / ...Method<Mesh>    -> same base / HipGridCharacteristicMethod
//   cubic::AbstractBorderConditions / BorderConditions       -> same base / HipBorderConditions
//   cubic::AbstractContactCopier / ContactCopier             -> same base / HipContactCopier
// The per-node work of stage(), border fills and contact copies runs on the GPU
// through include/gcmx.h; the host keeps set-up and the time loop.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gcmx.h"
#include "acoustic_model.hpp"
#include "snapshot.hpp"
#include "state_file.hpp"
#include "task.hpp"

namespace gcm {

/// engine/GlobalVariables.hpp:16-41 -- physical time and time step.
struct Clock {
	static real Time() { return time; }
	static real TimeStep() { return timeStep; }

private:
	static real time;
	static real timeStep;
	static void setZero() { time = timeStep = 0; }
	static void tickTack() { time += timeStep; }
	friend class AbstractEngine;
};

/// Throw gcm::Exception for a failed gcmx call.
void gcmxCheck(gcmx_status s, const char* what);

/// engine/AbstractEngine.hpp:29-55
class AbstractEngine {
public:
	explicit AbstractEngine(const Task& task);
	virtual ~AbstractEngine() = default;
	AbstractEngine(const AbstractEngine&) = delete;
	AbstractEngine& operator=(const AbstractEngine&) = delete;
	/// AbstractEngine::run (AbstractEngine.cpp:30-46)
	void run();
	/// `n` more time steps of the same loop body, ignoring requiredTime (benchmarks).
	void runSteps(int n);
	int stepsDone() const { return steps; }
	real getRequiredTime() const { return requiredTime; }
	/// The exact state of every body with the step count and the clock, to a file
	/// and back (state_file.hpp).  After loadState, run() continues the saved run:
	/// its step numbers go on from the restored count and the restored step's
	/// snapshots are not written again.  The cubic engine implements them.
	virtual void saveState(const std::string& path) const;
	virtual void loadState(const std::string& path);
	/// The file run() saves to (Task::Checkpoint); empty: none.
	std::string checkpointFile() const;

protected:
	const real CourantNumber = 0;
	real requiredTime = 0;
	int steps = 0;
	const Task::Checkpoint checkpoint;
	bool resumed = false;  // loadState restored `steps` and the clock; run() has not continued yet
	/// loadState's last act: the step count and the clock of the saved run.
	void restoreClock(int steps_, real time, real timeStep);
	void afterConstruction(const Task& task);
	virtual void nextTimeStep() = 0;
	virtual real estimateTimeStep() = 0;
	virtual void writeSnapshots(const int step) = 0;
	/// Snapshotter::flush of every snapshotter (the end of run()).
	virtual void flushSnapshots() const {}
};

/// grid/AbstractGrid.hpp -- what stage()/apply() receive and downcast.
class AbstractGrid {
public:
	virtual ~AbstractGrid() = default;
};

namespace cubic {

/// CubicGrid<D> (grid/cubic/CubicGrid.hpp) -- index arithmetic of the reference
/// storage order (X slowest); `it` are local indices, ghosts at -bs..-1 / size..
template <int D>
struct CubicGrid : public AbstractGrid {
	typedef std::array<int, D> IntD;
	typedef std::array<real, D> RealD;
	struct ConstructionPack {
		int borderSize = 0;
		IntD sizes{};
		IntD start{};
		RealD h{};
	};
	CubicGrid(size_t id_, const ConstructionPack& cp);
	size_t id;
	int borderSize;
	IntD sizes, start;
	RealD h;
	long long indexMaker[D];
	long long sizeOfAllNodes() const { return indexMaker[0] * (2LL * borderSize + sizes[0]); }
	long long getIndex(const IntD& it) const {
		long long a = 0;
		for (int i = 0; i < D; i++) a += indexMaker[i] * (long long)(it[i] + borderSize);
		return a;
	}
	/// coords (CubicGrid.hpp:114-126): startR + it * h, padded to 3-D
	Real3 coords(const IntD& it) const {
		Real3 c = {0, 0, 0};
		for (int i = 0; i < D; i++) c[i] = (real)start[i] * h[i] + (real)it[i] * h[i];
		return c;
	}
	real getMinimalSpatialStep() const;
	/// AABB in global indices {start, start + sizes - 1}
	std::pair<IntD, IntD> aabb() const;
};

/// engine/cubic/AbstractMesh.hpp:17-51
template <int D>
class AbstractMesh : public CubicGrid<D> {
public:
	using CubicGrid<D>::CubicGrid;
	virtual ~AbstractMesh() = default;
	virtual void setUpPde(const Task& task) = 0;
	virtual real getMaximalEigenvalue() const = 0;
	virtual void swapCurrAndNextPdeTimeLayer(int indexOfNextPde) = 0;
};

/// Host half of DefaultMesh::setUpPde (DefaultMesh.hpp:60-66): the PDE layer
/// after MaterialsCondition::apply + InitialCondition::apply in the reference
/// AoS all-nodes order, the material-condition index of every node (0 =
/// default, i = i-th area condition) and the GcmMatrices per condition.
/// No GPU involved; HipMesh::setUpPde uploads it.
template <int D>
struct HostState {
	std::vector<real> pde;
	std::vector<uint8_t> matId;
	std::vector<GcmMatrices<D>> matrices;
	/// An ACOUSTIC body (Task::Body::modelId): M = D + 1 components per node
	/// (velocity, then pressure) and AcousticModel matrices; `matrices` stays empty.
	Models::T model = Models::T::ELASTIC;
	int M = pdeSize(D);
	std::vector<AcousticMatrices<D>> acousticMatrices;
	size_t numberOfConditions() const { return model == Models::T::ACOUSTIC ? acousticMatrices.size() : matrices.size(); }
	std::vector<real> tau0;  // tau0 of the material (either kind) per material condition
	std::vector<int> materialNumber;  // its materialNumber per condition
	real maximalEigenvalue = 0;
};

/// Engine::createGridsAndContacts's ConstructionPack for body `id` (Engine.cpp:38-60).
template <int D>
typename CubicGrid<D>::ConstructionPack constructionPack(const Task& task, size_t id);

template <int D>
HostState<D> buildHostState(const Task& task, const CubicGrid<D>& grid);

/// The per-condition half of buildHostState: its HostState without the per-node
/// arrays (`pde` and `matId` empty), and the two lists its node loops apply --
/// the area of every material condition, and the (area, vector) pairs of
/// InitialCondition::apply in the reference's order: vectors, waves, quantities
/// (the first M entries of a vector count).
template <int D>
struct SetUpLists {
	HostState<D> st;
	std::vector<std::shared_ptr<Area>> materialAreas;
	std::vector<std::pair<std::shared_ptr<Area>, std::array<real, pdeSize(D)>>> initial;
};
template <int D>
SetUpLists<D> buildSetUpLists(const Task& task, const CubicGrid<D>& grid);

/// The per-node half: the two node loops of MaterialsCondition::apply and
/// InitialCondition::apply over the inner nodes of `grid`.  matId (zeros, the
/// grid's all-nodes size) takes the condition of every node; pde (zeros) takes
/// the state at layer.getIndex(it + shift), the node's place in the layer that
/// receives it: the grid itself, or the stack the grid is a member of.
/// buildHostState is buildSetUpLists followed by this.
template <int D>
void applySetUpLists(const SetUpLists<D>& ls, const CubicGrid<D>& grid, std::vector<uint8_t>& matId,
                     const CubicGrid<D>& layer, const std::array<int, D>& shift, std::vector<real>& pde);

/// One table over the material conditions of the bodies that share a context.
/// An entry views the matrices of a condition of either model (they stay in the
/// SetUpLists the table was built from).
template <int D>
struct MaterialTable {
	struct Entry {
		const real *U[D], *U1[D], *L[D];  // per axis: M * M, M * M and M values
		const void* bits;                 // the condition's whole matrices, to compare
		size_t nBits;
		real tau0, maximalEigenvalue;
	};
	int M = pdeSize(D);
	std::vector<Entry> entries;
	std::vector<std::vector<int>> entryOf;  // [member][condition] -> entry
};
/// `share`: bitwise-equal conditions (matrices and tau0) take one entry.
template <int D>
MaterialTable<D> buildMaterialTable(const std::vector<SetUpLists<D>>& lists, bool share);

/// An Area as the device knows it (gcmx_area); throws for a kind it does not.
gcmx_area deviceArea(const Area& area);

/// DefaultMesh's role with GPU-resident storage: the context owns both time
/// layers on the device; the host holds only set-up data.
///
/// SET-UP has one path, setUp(members, lists, onDevice), for the bodies that
/// share this mesh's context: the members of a stack, or the mesh itself as a
/// stack of one at offset 0 (setUpPde).  Every member first builds its matrices
/// and condition lists (setUpMember).  The path then makes one MaterialTable,
/// lets a node pass find the entries that hold inner nodes, sends those to the
/// device (sendMaterials), and lets the pass set the ids (only if more than one
/// material is in use) and the state.  The two passes differ in where the node
/// loops run: HostNodePass fills all-nodes arrays on the host and uploads one
/// layer; DeviceNodePass hands the members' areas to the device box by box and
/// allocates nothing the size of the grid.  DESIGN.md 3.6.1 lists the rules kept.
template <int D>
class HipMesh : public AbstractMesh<D> {
public:
	static constexpr int M = pdeSize(D);  ///< of an elastic body; an acoustic one holds pdeM() <= M
	typedef typename CubicGrid<D>::IntD IntD;
	/// The body's model (Task::Body::modelId) and the components per node it holds.
	Models::T model() const { return model_; }
	int pdeM() const { return pdeSizeOf(model_, D); }
	HipMesh(const Task& task, size_t id, const typename CubicGrid<D>::ConstructionPack& cp,
	        int device);
	~HipMesh() override;
	/// DefaultMesh::setUpPde (DefaultMesh.hpp:60-66): setUpMember, then setUp({this}).
	void setUpPde(const Task& task) override;
	real getMaximalEigenvalue() const override { return maximalEigenvalue; }
	/// The device swap happens inside gcmx_stage; nothing to do here.
	void swapCurrAndNextPdeTimeLayer(int) override {}
	gcmx_ctx* ctx() const { return ctx_; }
	/// Current layer in the reference AoS all-nodes order: readBox of the all-nodes
	/// box (a stack member reads its own part of the stack, no more).
	std::vector<real> pdeAll() const;
	/// The exact fp64 state of the nodes [boxMin, boxMax) as [node][pdeM()] in the
	/// reference's node order (gcmx_read_box / gcmx_write_box).  readBox may reach
	/// borderSize into the ghosts; writeBox takes inner nodes only and changes
	/// nothing else.  A stack member addresses the stack's context with its own
	/// offset, as snapshotArrays does.  stageBytes: bound of the device staging (0:
	/// the library's default).
	void readBox(const IntD& boxMin, const IntD& boxMax, real* aos, size_t stageBytes = 0) const;
	void writeBox(const IntD& boxMin, const IntD& boxMax, const real* aos, size_t stageBytes = 0);
	/// One node's PDE vector (gathers its pdeM() components on the device); an
	/// acoustic body fills the first pdeM() entries.
	std::array<real, M> pde(const IntD& it) const;

	/// OBSERVATION without a layer download (gcmx_gather / gcmx_snapshot_box).  Only
	/// inner nodes are asked for; a stack member addresses the stack's context with
	/// its own offset.  Quantities are PhysicalQuantities codes or GCMX_Q_COMPONENT(c).
	struct NodeList {  ///< inner nodes uploaded once (gcmx_node_list)
		gcmx_node_list* handle = nullptr;
		size_t size = 0;
		NodeList() = default;
		NodeList(const NodeList&) = delete;
		NodeList& operator=(const NodeList&) = delete;
		~NodeList() { gcmx_node_list_destroy(handle); }
	};
	std::shared_ptr<NodeList> nodeList(const std::vector<IntD>& nodes) const;
	/// [quantities][nodes] of the current layer.
	std::vector<real> gather(const NodeList& nodes, const std::vector<int>& quantities) const;
	/// The Float32 arrays of the inner box [boxMin, boxMax) in VTK point order (x
	/// fastest): velocity[n][3] (null: not wanted) and values[quantities][n].
	void snapshotArrays(const IntD& boxMin, const IntD& boxMax, const std::vector<int>& quantities,
	                    float* velocity, float* values) const;
	/// The same at every stride[d]-th node of the box (gcmx_snapshot_strided):
	/// ceil(extent / stride) points per axis, counted from boxMin.
	void snapshotArrays(const IntD& boxMin, const IntD& boxMax, const IntD& stride, const std::vector<int>& quantities,
	                    float* velocity, float* values) const;
	/// RECORDERS (gcmx_recorder): samples of the quantities at nodes, or at points
	/// in this mesh's inner-index units, kept on the device (record: no host wait)
	/// and read in batches.  Placed like nodeList: a stack member's receivers land
	/// at its offset in the stack's context.
	struct Recorder {
		gcmx_recorder* handle = nullptr;
		size_t receivers = 0, quantities = 0;
		Recorder() = default;
		Recorder(const Recorder&) = delete;
		Recorder& operator=(const Recorder&) = delete;
		~Recorder() { gcmx_recorder_destroy(handle); }
		int count() const { return gcmx_recorder_count(handle); }
	};
	std::shared_ptr<Recorder> recorder(const std::vector<IntD>& nodes, const std::vector<int>& quantities,
	                                   int capacity) const;
	std::shared_ptr<Recorder> recorder(const std::vector<std::array<real, D>>& points,
	                                   const std::vector<int>& quantities, int capacity) const;
	void record(Recorder& rec) const;
	/// Every sample held as [samples][quantities][receivers]; the recorder is empty afterwards.
	std::vector<real> readRecorder(Recorder& rec) const;
	/// Bytes the body's context copied {device -> host, host -> device} (gcmx_transfer_stats).
	std::array<uint64_t, 2> transferBytes() const;
	int numberOfMaterials() const { return (int)materialNumbers_.size(); }
	/// tau0 of the materials in the device table order (gcmx_set_materials).
	const std::vector<real>& deviceTau0() const { return deviceTau0_; }
	/// Material-condition index per node (all-nodes order) and the conditions'
	/// IsotropicMaterial::materialNumber (DefaultMesh::material(it), for snapshots).
	/// After a set-up on the device (Task::CubicGrid::setUpOnDevice) the ids come
	/// from the device on first use (gcmx_download_material_ids).
	const std::vector<uint8_t>& materialIdsAll() const {
		if (idsOnDevice_) fetchMaterialIds();
		return matIdAll_;
	}
	const std::vector<int>& materialNumbers() const { return materialNumbers_; }

	/// STACKS.  3-D bodies stacked along y or z whose every contact is an adhesion
	/// contact over a whole face (equal sizes and starts on the other two axes)
	/// run as ONE grid, the stack: ContactCopier::apply fills a body's ghost layers
	/// at the contact with the neighbour's current layer right before the stage of
	/// the contact's axis (Engine.cpp:99-107, ContactConditions.hpp:56-68) -- what
	/// the stack's stage reads there anyway -- so every inner node is bitwise that
	/// of the separate bodies (TestEngine.cpp:27-87 pins split == unsplit), and the
	/// step keeps the one-pass kernel instead of three per-stage passes.  A member
	/// keeps its own host data (materials, snapshots) and reads its part of the
	/// stack's device layers; the stack is a HipMesh over the combined box, set up
	/// from its members' lists (setUp).  A member's ghost layers at a contact are
	/// its neighbour's inner layers.
	void joinStack(const std::shared_ptr<HipMesh<D>>& stack, int axis, int offset);
	const std::shared_ptr<HipMesh<D>>& stackMesh() const { return stack_; }
	/// The per-condition half of a body's set-up (its own or a stack member's):
	/// the lists, its eigenvalue over ALL its conditions, its material numbers.
	SetUpLists<D> setUpMember(const Task& task);
	/// The set-up of this mesh's context from the bodies in it, in stack order,
	/// with the node loops on the host or on the device (see the class comment).
	void setUp(const std::vector<HipMesh<D>*>& members, const std::vector<SetUpLists<D>>& lists, bool onDevice);

private:
	std::shared_ptr<HipMesh<D>> stack_;  // set for a stack member
	int stackAxis_ = -1, stackOffset_ = 0;
	bool ownsCtx_ = true;
	gcmx_ctx* ctx_ = nullptr;
	int device;
	real maximalEigenvalue = 0;
	Models::T model_ = Models::T::ELASTIC;
	std::vector<real> deviceTau0_;
	mutable std::vector<uint8_t> matIdAll_;
	std::vector<int> materialNumbers_;  // one per material condition
	bool pdeIsSetUp = false;
	void markSetUp();  // throws the second time
	/// PLACEMENT.  A node of this mesh as a node of its context: a stack member
	/// lies stackOffset_ nodes along stackAxis_.
	IntD inContext(IntD it) const {
		if (stack_) it[stackAxis_] += stackOffset_;
		return it;
	}
	/// The box [boxMin, boxMax) of this mesh as a box of its context; throws
	/// `refusal` where it leaves [-reach, size + reach) on an axis.
	struct PlacedBox {
		int lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
	};
	PlacedBox placeBox(const IntD& boxMin, const IntD& boxMax, int reach, const char* refusal) const;
	/// This mesh's inner nodes as a box of its context, with its own start.
	gcmx_setup_box setupBox() const;
	/// The used entries of a table to the device (gcmx_set_materials) and their
	/// tau0 to deviceTau0_; entry -> device id, -1 for an unused one.
	std::vector<int> sendMaterials(const MaterialTable<D>& table, const std::vector<int>& used);
	struct NodePass;  // census() before the table is sent, place(dev) after
	struct HostNodePass;
	struct DeviceNodePass;
	// set-up on the device: the ids wait on the device until a snapshot asks
	void fetchMaterialIds() const;
	mutable bool idsOnDevice_ = false;
	std::vector<std::shared_ptr<Area>> materialAreas_;  // per condition, for fetchMaterialIds
	std::vector<int> conditionOfDeviceId_;               // device id -> condition, -1: none, -2: several
};

/// engine/cubic/GridCharacteristicMethod.hpp:13-17
class GridCharacteristicMethodBase {
public:
	virtual ~GridCharacteristicMethodBase() = default;
	virtual void stage(const int s, const real& timeStep, AbstractGrid& mesh) const = 0;
};

/// GridCharacteristicMethod<Mesh>::stage on the device (gcmx_stage).
template <int D>
class HipGridCharacteristicMethod : public GridCharacteristicMethodBase {
public:
	explicit HipGridCharacteristicMethod(const Task&) {}
	void stage(const int s, const real& timeStep, AbstractGrid& mesh) const override;
	/// All D stages at once (gcmx_step; fused kernels where admissible).
	void step(const real& timeStep, HipMesh<D>& mesh) const;
};

/// engine/cubic/BorderConditions.hpp:17-20
class AbstractBorderConditions {
public:
	virtual ~AbstractBorderConditions() = default;
	virtual void apply(AbstractGrid& mesh, const int direction) const = 0;
	virtual bool empty() const = 0;
	/// Every face uniform: each node of a face has the same last-applying
	/// condition, or none has any (then gcmx_step_faces runs the whole step).
	virtual bool uniformFaces() const { return false; }
	/// gcmx_face per face (2*D entries, faces[2*axis + side]) at Clock::Time().
	virtual void faces(gcmx_face*) const {}
	/// Non-uniform faces held as a per-node face map (gcmx_face_map): the whole
	/// step runs through gcmx_step_face_map.  Null when there is none.
	virtual const gcmx_face_map* faceMap() const { return nullptr; }
	/// Every condition's quantities at Clock::Time() (the face map's conditions).
	virtual int conditionsAt(gcmx_face*) const { return 0; }
};

/// BorderConditions<Mesh> (BorderConditions.hpp:23-121): node lists found on the
/// host at construction (:46-78) and uploaded to the device once; ghost fills
/// on the device per stage (:81-114), enqueued without host synchronisation.
/// When every face is uniform the engine runs whole steps (gcmx_step_faces).
template <int D>
class HipBorderConditions : public AbstractBorderConditions {
public:
	HipBorderConditions(const Task& task, const HipMesh<D>& mesh);
	~HipBorderConditions() override;
	HipBorderConditions(const HipBorderConditions&) = delete;
	HipBorderConditions& operator=(const HipBorderConditions&) = delete;
	void apply(AbstractGrid& mesh, const int direction) const override;
	bool empty() const override { return conditions.empty(); }
	bool uniformFaces() const override { return uniform; }
	void faces(gcmx_face* out) const override;
	const gcmx_face_map* faceMap() const override { return faceMap_; }
	int conditionsAt(gcmx_face* out) const override;

private:
	struct Condition {
		int direction;
		std::vector<int> leftNodes, rightNodes;  // D ints per node
		gcmx_border_nodes* leftD = nullptr;      // the same lists on the device
		gcmx_border_nodes* rightD = nullptr;
		std::vector<std::pair<PhysicalQuantities::T, Task::TimeDependency>> values;
	};
	std::vector<Condition> conditions;
	bool uniform = false;
	std::array<int, 6> faceCondition{{-1, -1, -1, -1, -1, -1}};  // per face: condition or -1
	gcmx_face_map* faceMap_ = nullptr;  // non-uniform faces, <= GCMX_MAX_FACE_CONDITIONS conditions
};

/// engine/cubic/ContactConditions.hpp:20-68 (adhesion: plain copy)
template <int D>
class HipContactCopier {
public:
	HipContactCopier(const std::array<int, 3>& dstMin, const std::array<int, 3>& dstMax,
	                 const std::array<int, 3>& srcMin)
	    : dmin(dstMin), dmax(dstMax), smin(srcMin) {}
	void apply(HipMesh<D>& a, const HipMesh<D>& b) const;

private:
	std::array<int, 3> dmin, dmax, smin;
};

/// rheology/ode/Ode.hpp:16-19
class AbstractOde {
public:
	virtual ~AbstractOde() = default;
	virtual void apply(AbstractGrid& mesh, const real timeStep) = 0;
};

/// MaxwellViscosityOde<Mesh> (rheology/ode/Ode.hpp:24-38) on the device:
/// sigma *= exp(-timeStep / tau0) per node (gcmx_ode_maxwell).
template <int D>
class HipMaxwellViscosityOde : public AbstractOde {
public:
	void apply(AbstractGrid& mesh, const real timeStep) override;
};

/// VtkSnapshotter<Mesh> (util/snapshot/VtkSnapshotter.hpp:12-86): one .vts per
/// snapshot under snapshots[/outDir]/vtk/.
template <int D>
class VtkSnapshotter : public Snapshotter {
public:
	explicit VtkSnapshotter(const Task& task)
	    : Snapshotter(task), quantitiesToSnap(task.vtkSnapshotter.quantitiesToSnap),
	      chunkBytes(task.vtkSnapshotter.chunkBytes), settings(task.vtkSnapshotter) {}

protected:
	/// The file's Velocity and quantity arrays come from the device already as
	/// Float32 in VTK order (HipMesh::snapshotArrays), in slabs along the slowest VTK
	/// axis of at most chunkBytes of output each.  With Task::vtkSnapshotter.stride
	/// or .box the file holds the selected nodes only (VtkSelection), the slabs are
	/// counted in output indices, and a body the box misses writes no file.
	void snapshotImpl(const AbstractGrid* mesh, const int step) override;

private:
	const std::vector<PhysicalQuantities::T> quantitiesToSnap;
	const size_t chunkBytes;
	const Task::VtkSnapshotter settings;
};

/// SliceSnapshotter<Mesh> (util/snapshot/SliceSnapshotter.hpp:12-118): velocity
/// along the last axis through the centre into snapshots/../zaxis/*.txt, and the
/// mean detector quantity over the top face (last axis) into ../detector/*.txt.
template <int D>
class SliceSnapshotter : public Snapshotter {
public:
	explicit SliceSnapshotter(const Task& task);
	/// Task::Detector::bufferSteps > 0: the snapshots still on the device, written
	/// as the files the unbuffered run writes.
	void flush() override;

protected:
	void snapshotImpl(const AbstractGrid* mesh, const int step) override;

private:
	size_t gridId;
	std::vector<real> times, seismo;
	/// Buffered: the recorders of the two node lists and the step and time of
	/// every sample they hold.
	int bufferSteps = 0;
	std::shared_ptr<typename HipMesh<D>::Recorder> columnRec, detectorRec;
	std::vector<int> heldSteps;
	std::vector<real> heldTimes;
	void writeFiles(const HipMesh<D>* mesh, int step, real time, const real* Vz, const real* valuesInArea,
	                size_t nValues);
	std::shared_ptr<Area> detectionArea;
	PhysicalQuantities::T quantityToWrite;
	/// Made on first use, gathered at every snapshot: the column through sizes / 2
	/// and the top-face nodes inside the detection area (forEachInner order).
	const HipMesh<D>* listsOf = nullptr;
	std::shared_ptr<typename HipMesh<D>::NodeList> column, detector;
};

/// Snapshotters::T::DETECTOR, which the reference declares (util/Enum.hpp:140) and
/// never builds: seismograms at Task::Receivers' points of body gridId (other
/// bodies: nothing).  A point p is position (p_d - coords(0)_d) / h_d in inner-index
/// units; one outside the body's inner nodes throws at the first snapshot.  One
/// sample per snapshot step goes to a device recorder; every bufferSteps samples
/// and at flush() one text file snapshots[/outDir]/receivers/mesh<id>core00snap<step
/// of its first row>.txt is written: per row the time, then the quantities x
/// receivers values in quantity-major order, tab-separated, printed with %.17g.
/// The files in step order are the whole record; none is reopened.
template <int D>
class ReceiverSnapshotter : public Snapshotter {
public:
	explicit ReceiverSnapshotter(const Task& task);
	void flush() override;

protected:
	void snapshotImpl(const AbstractGrid* mesh, const int step) override;

private:
	const Task::Receivers settings;
	const HipMesh<D>* mesh = nullptr;
	std::shared_ptr<typename HipMesh<D>::Recorder> rec;
	std::vector<int> heldSteps;
	std::vector<real> heldTimes;
};

/// engine/cubic/AbstractFactory.hpp:22-54
template <int D>
class AbstractFactoryBase {
public:
	virtual ~AbstractFactoryBase() = default;
	virtual std::shared_ptr<AbstractMesh<D>> createMesh(
	    const Task& task, size_t gridId, const typename CubicGrid<D>::ConstructionPack& cp,
	    size_t numberOfNextPdeTimeLayers) = 0;
	virtual std::shared_ptr<GridCharacteristicMethodBase> createGcm(const Task& task) = 0;
	virtual std::shared_ptr<AbstractBorderConditions> createBorder(
	    const Task& task, std::shared_ptr<AbstractMesh<D>> mesh) = 0;
	virtual std::shared_ptr<AbstractOde> createOde(const Odes::T type) = 0;
	virtual std::shared_ptr<Snapshotter> createSnapshotter(const Task& task,
	                                                       const Snapshotters::T type) = 0;
};

/// AbstractFactory<ElasticModel<D>, CubicGrid<D>, IsotropicMaterial, HipMesh>; a body whose
/// Task::Body::materialId is ORTHOTROPIC is built with OrthotropicMaterial, one whose
/// modelId is ACOUSTIC with AcousticModel<D> (buildHostState): the three products of
/// Engine<D>::createAbstractFactory (engine/cubic/Engine.cpp:155-189)
template <int D>
class HipFactory : public AbstractFactoryBase<D> {
public:
	explicit HipFactory(int device_) : device(device_) {}
	std::shared_ptr<AbstractMesh<D>> createMesh(const Task& task, size_t gridId,
	                                            const typename CubicGrid<D>::ConstructionPack& cp,
	                                            size_t) override {
		return std::make_shared<HipMesh<D>>(task, gridId, cp, device);
	}
	std::shared_ptr<GridCharacteristicMethodBase> createGcm(const Task& task) override {
		return std::make_shared<HipGridCharacteristicMethod<D>>(task);
	}
	std::shared_ptr<AbstractBorderConditions> createBorder(
	    const Task& task, std::shared_ptr<AbstractMesh<D>> mesh) override {
		return std::make_shared<HipBorderConditions<D>>(
		    task, dynamic_cast<const HipMesh<D>&>(*mesh));
	}
	/// AbstractFactory.hpp:90-93: every ODE type maps to MaxwellViscosityOde there;
	/// the other two do not compile in the reference (Ode.hpp:50, 75), so they are
	/// refused here.
	std::shared_ptr<AbstractOde> createOde(const Odes::T type) override {
		if (type != Odes::T::MAXWELL_VISCOSITY)
			throw Exception("only the Maxwell viscosity ODE is on this path");
		return std::make_shared<HipMaxwellViscosityOde<D>>();
	}
	/// AbstractFactory.hpp:95-105
	std::shared_ptr<Snapshotter> createSnapshotter(const Task& task,
	                                               const Snapshotters::T type) override {
		switch (type) {
		case Snapshotters::T::VTK: return std::make_shared<VtkSnapshotter<D>>(task);
		case Snapshotters::T::SLICESNAP: return std::make_shared<SliceSnapshotter<D>>(task);
		case Snapshotters::T::DETECTOR: return std::make_shared<ReceiverSnapshotter<D>>(task);
		default: throw Exception("Unknown or unsupported snapshotter");
		}
	}

private:
	int device;
};

/// cubic::Engine<D> (engine/cubic/Engine.{hpp,cpp})
template <int D>
class Engine : public AbstractEngine {
public:
	typedef CubicGrid<D> Grid;
	explicit Engine(const Task& task, int device = 0);
	/// Flushes the snapshotters (what they still hold on the device); never throws.
	~Engine() override;
	std::shared_ptr<const HipMesh<D>> getMesh(size_t gridId) const;
	/// saveState streams every body's inner nodes in slabs along x of at most
	/// Task::vtkSnapshotter.chunkBytes (one x plane at least) through readBox to a
	/// temporary file and renames it; loadState validates the whole file against
	/// the engine's bodies first (a mismatch throws and leaves the engine as it
	/// was), then streams writeBox and restores the step count and the clock.
	void saveState(const std::string& path) const override;
	void loadState(const std::string& path) override;

protected:
	void nextTimeStep() override;
	real estimateTimeStep() override;
	void writeSnapshots(const int step) override;
	void flushSnapshots() const override;

private:
	struct Body {
		std::shared_ptr<AbstractFactoryBase<D>> factory;
		std::shared_ptr<AbstractMesh<D>> mesh;
		std::shared_ptr<HipMesh<D>> stack;  // the stack this body belongs to (HipMesh::joinStack)
		bool stackLead = false;             // the member that steps the stack
		std::shared_ptr<GridCharacteristicMethodBase> gcm;
		std::shared_ptr<AbstractBorderConditions> border;
		struct Contact {
			size_t neighborId;
			int direction;
			std::shared_ptr<HipContactCopier<D>> copier;
		};
		std::vector<Contact> contacts;
		std::vector<std::shared_ptr<AbstractOde>> odes;
		std::vector<std::shared_ptr<Snapshotter>> snapshotters;
	};
	std::vector<Body> bodies;
	std::map<size_t, std::vector<size_t>> stackOrder_;  // lead id -> member ids along the stack axis
	int device;
	Body& getBody(size_t id);
	const Body& getBody(size_t id) const;
	void createGridsAndContacts(const Task& task);
	void buildStacks(const Task& task);
	/// The mesh a body's step runs on: its own, its stack's (the lead member), or
	/// none (the other members of a stack).
	HipMesh<D>* unitMesh(Body& b);
	void applyOdes();
	const size_t stateChunkBytes;  // Task::vtkSnapshotter.chunkBytes
	StateFileHeader stateHeader() const;
};

}  // namespace cubic

/// engine/EngineFactory.hpp:11-38 (cubic only on this path)
std::shared_ptr<AbstractEngine> createEngine(const Task& task, int device = 0);

}  // namespace gcm
