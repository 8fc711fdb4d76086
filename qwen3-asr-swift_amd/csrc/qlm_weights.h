// qlm_weights.h -- the checked weight loader of the quantised speech LMs (the Qwen3-TTS Talker and code predictor, the CosyVoice3
// speech-token LLM): float tensors to bf16, MLX affine 4 / 8 bit Linears (dec_quant.h) fused row-wise, and the device buffers they
// land in.  Every refusal is a WeightLoadError whose message starts with "<who>: ": QASR_ERR_IO for a missing key, QASR_ERR_INVALID
// otherwise.  A dry loader runs the host checks alone: no HIP call, null pointers in what it returns.
#pragma once
#include "engine.h"
#include "dec_quant.h"
#include "safetensors.h"
#include <memory>
#include <set>
#include <string>
#include <vector>

namespace qasr {

struct QLin { QuantImg img; const float* bias = nullptr; int N = 0, K = 0; };   // N: rows of the checkpoint (img.raw.N: with the zero rows)

enum class QlmBias { NONE, F32, BF16 };   // the Linear bias `<stem>.bias` of every stem: widened to f32 | each value rounded through bf16

class QlmLoader {
  public:
    QlmLoader(const char* who, hipStream_t stream, bool dry) : who_(who), stream_(stream), dry_(dry) {}
    bool dry() const { return dry_; }
    // the arena: a buffer of `bytes` that lives as long as the loader, filled from src unless that is null
    void* upload(const void* src, size_t bytes);
    size_t param_bytes() const { return param_bytes_; }        // bytes of the tensors read, as the checkpoint stores them
    size_t device_bytes() const { return device_bytes_; }
    const bf16_t* bf16(const SafeTensorsDir& st, const std::string& key, std::vector<int64_t> shape);
    // One quantised Linear, or several fused row-wise: stems concatenated (q | k | v), or two stems interleaved in blocks of `interleave`
    // rows (gate | up, the layout the SWIGLU epilogues read).  pad_to: zero rows up to that many.  The raw triplet only: see pack().
    QLin qlin(const SafeTensorsDir& st, const std::vector<std::string>& stems, int K, int bits, QlmBias bias = QlmBias::NONE,
              int interleave = 0, int pad_to = 0);
    void pack(QLin& q);                                        // the packed images of dec_quant.h (quant_pack_launch) next to the triplet
    void mark_seen(const std::string& key) { seen_.insert(key); }
    void refuse_unexpected(const SafeTensorsDir& st) const;    // the first key of st (map order) that was neither read nor marked
    [[noreturn]] void refuse(const std::string& what) const;   // WeightLoadError(QASR_ERR_INVALID, "<who>: " + what)

  private:
    const SafeEntry& need(const SafeTensorsDir& st, const std::string& key);
    std::string who_;
    hipStream_t stream_;
    bool dry_;
    size_t param_bytes_ = 0, device_bytes_ = 0;
    std::vector<std::unique_ptr<DevBuf>> bufs_;
    std::set<std::string> seen_;
};

// One decoder layer under the key prefix p ("...layers.3."): q|k|v fused, o, gate|up interleaved by 16, down, the two norms; refuses
// row counts that do not match the geometry.  Nothing is packed.
struct QlmLayer { QLin qkv, o, gu, down; const bf16_t *ln1 = nullptr, *ln2 = nullptr; };
struct QlmLayerGeom { int H, nq, nkv, I, bits; };              // hidden, query and key / value widths (heads * head_dim), intermediate
QlmLayer qlm_load_layer(QlmLoader& wl, const SafeTensorsDir& st, const std::string& p, const QlmLayerGeom& g, QlmBias qkv_bias);

}  // namespace qasr
