// state_file.cpp -- the GPU-free half of the engine's state file (state_file.hpp).
#include "state_file.hpp"

#include <cstring>

#include "snapshot.hpp"

namespace gcm {

namespace {

const char kMagic[8] = {'G', 'C', 'M', 'X', 'S', 'T', 'A', 'T'};

// little-endian, whatever the host's order
void put(unsigned char* p, uint64_t v, int bytes) {
	for (int i = 0; i < bytes; i++) p[i] = (unsigned char)(v >> (8 * i));
}
uint64_t get(const unsigned char* p, int bytes) {
	uint64_t v = 0;
	for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
	return v;
}
uint64_t bitsOf(real x) {
	uint64_t u;
	static_assert(sizeof(u) == sizeof(x), "real is fp64");
	std::memcpy(&u, &x, sizeof(u));
	return u;
}
real realOf(uint64_t u) {
	real x;
	std::memcpy(&x, &u, sizeof(x));
	return x;
}

std::string sizesText(const std::array<uint32_t, 3>& s) {
	return std::to_string(s[0]) + "x" + std::to_string(s[1]) + "x" + std::to_string(s[2]);
}

}  // namespace

std::vector<uint64_t> stateFileOffsets(const StateFileHeader& h) {
	std::vector<uint64_t> off;
	uint64_t at = kStateHeaderBytes;
	for (const StateFileBody& b : h.bodies) {
		at += kStateBodyRecordBytes;
		off.push_back(at);
		at += b.dataBytes();
	}
	off.push_back(at);
	return off;
}

StateFileHeader readStateFileHeader(const std::string& path) {
	std::FILE* f = std::fopen(path.c_str(), "rb");
	if (!f) throw Exception("state file " + path + ": cannot open");
	struct Close {
		std::FILE* f;
		~Close() { std::fclose(f); }
	} closer{f};
	const std::string where = "state file " + path + ": ";
	if (std::fseek(f, 0, SEEK_END) != 0) throw Exception(where + "cannot seek");
	const long long fileSize = std::ftell(f);
	if (fileSize < 0) throw Exception(where + "cannot tell its size");
	std::rewind(f);
	unsigned char hd[kStateHeaderBytes];
	if ((uint64_t)fileSize < kStateHeaderBytes || std::fread(hd, 1, sizeof(hd), f) != sizeof(hd))
		throw Exception(where + "truncated: size " + std::to_string(fileSize) + " is shorter than the header");
	if (std::memcmp(hd, kMagic, 8) != 0) throw Exception(where + "magic: not a state file");
	const uint32_t version = (uint32_t)get(hd + 8, 4);
	if (version != kStateFileVersion)
		throw Exception(where + "version: " + std::to_string(version) + ", this build reads " + std::to_string(kStateFileVersion));
	StateFileHeader h;
	h.D = (uint32_t)get(hd + 12, 4);
	if (h.D < 1 || h.D > 3) throw Exception(where + "D: " + std::to_string(h.D) + " is not 1..3");
	const uint64_t count = get(hd + 16, 8);
	h.steps = (int64_t)get(hd + 24, 8);
	h.time = realOf(get(hd + 32, 8));
	h.timeStep = realOf(get(hd + 40, 8));
	if (h.steps < 0) throw Exception(where + "steps: negative");
	// every body takes a record at least, so the count is bounded by the size
	if (count < 1 || count > ((uint64_t)fileSize - kStateHeaderBytes) / kStateBodyRecordBytes)
		throw Exception(where + "body count: " + std::to_string(count) + " does not fit a file of " +
		                std::to_string(fileSize) + " bytes (truncated?)");
	uint64_t at = kStateHeaderBytes;
	for (uint64_t k = 0; k < count; k++) {
		const std::string body = "body " + std::to_string(k) + ": ";
		unsigned char rec[kStateBodyRecordBytes];
		if (at + kStateBodyRecordBytes > (uint64_t)fileSize || std::fseek(f, (long)at, SEEK_SET) != 0 ||
		    std::fread(rec, 1, sizeof(rec), f) != sizeof(rec))
			throw Exception(where + body + "truncated: the record at " + std::to_string(at) + " is past the size " +
			                std::to_string(fileSize));
		StateFileBody b;
		b.id = get(rec, 8);
		const uint32_t model = (uint32_t)get(rec + 8, 4);
		if (model > (uint32_t)Models::T::ACOUSTIC) throw Exception(where + body + "model: unknown code " + std::to_string(model));
		b.model = (Models::T)model;
		b.M = (uint32_t)get(rec + 12, 4);
		if (b.M < 1 || b.M > 9) throw Exception(where + body + "M: " + std::to_string(b.M) + " is not 1..9");
		for (int d = 0; d < 3; d++) {
			b.sizes[d] = (uint32_t)get(rec + 16 + 4 * d, 4);
			if (b.sizes[d] < 1 || b.sizes[d] > (1u << 30) || (d >= (int)h.D && b.sizes[d] != 1))
				throw Exception(where + body + "sizes: " + sizesText(b.sizes) + " is no " + std::to_string(h.D) + "-D grid");
		}
		at += kStateBodyRecordBytes;
		if (b.dataBytes() > (uint64_t)fileSize - at)
			throw Exception(where + body + "truncated: " + std::to_string(b.dataBytes()) + " bytes of nodes at " +
			                std::to_string(at) + " do not fit the size " + std::to_string(fileSize));
		at += b.dataBytes();
		h.bodies.push_back(b);
	}
	if (at != (uint64_t)fileSize)
		throw Exception(where + "size: " + std::to_string(fileSize) + " bytes, its records say " + std::to_string(at));
	return h;
}

void checkStateFileHeader(const StateFileHeader& file, const StateFileHeader& engine) {
	if (file.D != engine.D)
		throw Exception("state file: D: the file has " + std::to_string(file.D) + ", the engine " + std::to_string(engine.D));
	if (file.bodies.size() != engine.bodies.size())
		throw Exception("state file: body count: the file has " + std::to_string(file.bodies.size()) + ", the engine " +
		                std::to_string(engine.bodies.size()));
	for (size_t k = 0; k < file.bodies.size(); k++) {
		const StateFileBody &a = file.bodies[k], &b = engine.bodies[k];
		const std::string body = "state file: body " + std::to_string(k) + ": ";
		if (a.id != b.id) throw Exception(body + "id: the file has " + std::to_string(a.id) + ", the engine " + std::to_string(b.id));
		if (a.model != b.model)
			throw Exception(body + "model: the file has " + std::to_string((int)a.model) + ", the engine " +
			                std::to_string((int)b.model) + " (0 elastic, 1 acoustic)");
		if (a.M != b.M) throw Exception(body + "M: the file has " + std::to_string(a.M) + ", the engine " + std::to_string(b.M));
		if (a.sizes != b.sizes)
			throw Exception(body + "sizes: the file has " + sizesText(a.sizes) + ", the engine " + sizesText(b.sizes));
	}
}

StateFileWriter::StateFileWriter(const std::string& path) : path_(path), tmp_(path + ".tmp") {
	makeParentDirectories(path_);
	f_ = std::fopen(tmp_.c_str(), "wb");
	if (!f_) throw Exception("state file " + tmp_ + ": cannot open for writing");
}

StateFileWriter::~StateFileWriter() {
	if (!f_) return;  // committed
	std::fclose(f_);
	std::remove(tmp_.c_str());
}

void StateFileWriter::write(const void* data, size_t bytes) {
	if (!f_) throw Exception("state file " + path_ + ": written after commit");
	if (std::fwrite(data, 1, bytes, f_) != bytes) throw Exception("state file " + tmp_ + ": write failed");
	written_ += bytes;
}

void StateFileWriter::writeHeader(const StateFileHeader& h) {
	unsigned char hd[kStateHeaderBytes];
	std::memcpy(hd, kMagic, 8);
	put(hd + 8, kStateFileVersion, 4);
	put(hd + 12, h.D, 4);
	put(hd + 16, h.bodies.size(), 8);
	put(hd + 24, (uint64_t)h.steps, 8);
	put(hd + 32, bitsOf(h.time), 8);
	put(hd + 40, bitsOf(h.timeStep), 8);
	write(hd, sizeof(hd));
}

void StateFileWriter::writeBodyRecord(const StateFileBody& b) {
	unsigned char rec[kStateBodyRecordBytes];
	put(rec, b.id, 8);
	put(rec + 8, (uint64_t)b.model, 4);
	put(rec + 12, b.M, 4);
	for (int d = 0; d < 3; d++) put(rec + 16 + 4 * d, b.sizes[d], 4);
	put(rec + 28, 0, 4);
	write(rec, sizeof(rec));
}

void StateFileWriter::commit() {
	if (!f_) throw Exception("state file " + path_ + ": committed twice");
	const bool ok = std::fflush(f_) == 0;
	const bool closed = std::fclose(f_) == 0;
	f_ = nullptr;
	if (!ok || !closed) {
		std::remove(tmp_.c_str());
		throw Exception("state file " + tmp_ + ": write failed");
	}
	if (std::rename(tmp_.c_str(), path_.c_str()) != 0) {
		std::remove(tmp_.c_str());
		throw Exception("state file " + path_ + ": rename failed");
	}
}

}  // namespace gcm
