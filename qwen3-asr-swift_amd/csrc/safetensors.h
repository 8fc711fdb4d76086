// safetensors.h -- sharded safetensors directory reader shared by the Qwen3-ASR and the Omnilingual loaders.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace qasr {

struct SafeEntry {
    std::string dtype;                 // "F32" | "F16" | "BF16" | "U32" | ...
    std::vector<int64_t> shape;
    const uint8_t* data;               // inside a mapping owned by the SafeTensorsDir
    size_t bytes;
    size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};

// element i of a float tensor (F32 / F16 / BF16) as f32
float safe_elem_f32(const SafeEntry& e, size_t i);

class SafeTensorsDir {
public:
    // maps every *.safetensors of the directory (only_file given: that one file of it), validates the headers
    explicit SafeTensorsDir(const std::string& dir, const std::string& only_file = "");
    ~SafeTensorsDir();
    std::map<std::string, SafeEntry> entries;
private:
    struct Mapping;
    std::vector<std::unique_ptr<Mapping>> maps_;
};

// A small model's whole checkpoint (Silero VAD, WeSpeaker), widened to f32 in the reference's layouts.
struct CheckedWeights {
    std::map<std::string, std::vector<float>> t;
    size_t disk_bytes = 0;                          // parameter bytes as stored (memoryFootprint)
};
struct WeightLoadError : std::runtime_error {      // code: QASR_ERR_IO (missing file / key) or QASR_ERR_INVALID (shape / dtype / unknown key)
    int code;
    WeightLoadError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
// reads <dir>/<file> (model.safetensors unless named; a named file is read alone, the directory's other files are left out) against a key -> shape table: presence, shape and dtype (F32 / F16 / BF16) of every entry, unknown keys
// refused on request; messages start with "<who>: ".  Host work only: no HIP call.  optional_default: for a key the file lacks, the
// value (>= 0) the reference's module holds before loading, which then fills the tensor; a negative answer (or no function) makes the
// key required.
CheckedWeights load_checked_f32(const std::string& dir, const char* who,
                                const std::vector<std::pair<std::string, std::vector<int64_t>>>& shapes, bool refuse_unknown_keys,
                                float (*optional_default)(const std::string&) = nullptr, const char* file = nullptr);
// the same checks over an opened directory: for a checkpoint whose tensors lie in any of the directory's *.safetensors files
CheckedWeights load_checked_f32(const SafeTensorsDir& dir, const char* who,
                                const std::vector<std::pair<std::string, std::vector<int64_t>>>& shapes, bool refuse_unknown_keys,
                                float (*optional_default)(const std::string&) = nullptr);

}  // namespace qasr
