// state_file.hpp -- the file Engine::saveState writes and Engine::loadState
// reads: the exact fp64 state of every body with the step count and the clock,
// enough for a fresh engine built from the same task to continue bit for bit.
// This is the GPU-free half (header, offsets, validation, the temporary name and
// the rename); the engine streams the bodies through HipMesh::readBox / writeBox.
//
// Little-endian throughout.
//   engine header, 48 bytes:
//     char[8]  "GCMXSTAT"
//     uint32   format version (1)
//     uint32   D
//     uint64   number of bodies
//     int64    steps
//     uint64   bits of Clock::time
//     uint64   bits of Clock::timeStep
//   then per body, in the engine's body order:
//     body record, 32 bytes:
//       uint64   id
//       uint32   model (Models::T)
//       uint32   M, components per node
//       uint32   sizes[3] (1 for axes >= D)
//       uint32   0
//     the body's inner nodes as raw fp64, [node][M], the reference's node order
//     (x slowest, last axis fastest): sizes[0] * sizes[1] * sizes[2] * M * 8 bytes.
#pragma once

#include <array>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "task.hpp"

namespace gcm {

constexpr uint32_t kStateFileVersion = 1;
constexpr uint64_t kStateHeaderBytes = 48, kStateBodyRecordBytes = 32;

struct StateFileBody {
	uint64_t id = 0;
	Models::T model = Models::T::ELASTIC;
	uint32_t M = 0;
	std::array<uint32_t, 3> sizes{{1, 1, 1}};
	uint64_t nodes() const { return (uint64_t)sizes[0] * sizes[1] * sizes[2]; }
	uint64_t dataBytes() const { return nodes() * M * sizeof(real); }
};

struct StateFileHeader {
	uint32_t D = 0;
	int64_t steps = 0;
	real time = 0, timeStep = 0;
	std::vector<StateFileBody> bodies;
};

/// Byte offset of every body's data (its record ends there), then the file's size.
std::vector<uint64_t> stateFileOffsets(const StateFileHeader& h);

/// Parse and check the file's own consistency: magic, version, D in 1..3, M and
/// sizes plausible, every record where the ones before put it, and the file
/// exactly as long as its records say.  Throws gcm::Exception naming the field.
StateFileHeader readStateFileHeader(const std::string& path);

/// The file's header against what the engine holds (its `steps` and clock are
/// not compared): D, the body count, then per body id, model, M and sizes.
/// Throws gcm::Exception naming the field and the body.
void checkStateFileHeader(const StateFileHeader& file, const StateFileHeader& engine);

/// Writes `path` + ".tmp" and renames it to `path` in commit(), so an
/// interrupted save never leaves a short file under the final name (a previous
/// file there stays until the rename replaces it).  Without commit() the
/// destructor removes the temporary file.
class StateFileWriter {
public:
	explicit StateFileWriter(const std::string& path);
	~StateFileWriter();
	StateFileWriter(const StateFileWriter&) = delete;
	StateFileWriter& operator=(const StateFileWriter&) = delete;
	const std::string& temporaryPath() const { return tmp_; }
	/// The engine header; h.bodies gives the count only.
	void writeHeader(const StateFileHeader& h);
	void writeBodyRecord(const StateFileBody& b);
	void write(const void* data, size_t bytes);
	uint64_t written() const { return written_; }
	void commit();

private:
	std::string path_, tmp_;
	std::FILE* f_ = nullptr;
	uint64_t written_ = 0;
};

}  // namespace gcm
