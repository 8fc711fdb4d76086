// qlm_loader_check.cpp -- the shared weight loader's host pass (csrc/qlm_weights.cpp, dry mode) as a program of its own, for a run
// under the host sanitizers: no device, nothing loaded into another process.  Build and run from qwen3-asr-swift_amd/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../include -Icsrc -Xarch_host -fsanitize=address,undefined \
//         -ffunction-sections -Wl,--gc-sections -x hip ../tools/qlm_loader_check.cpp csrc/qlm_weights.cpp csrc/safetensors.cpp \
//         -o build/qlm_loader_check
//   build/qlm_loader_check <dir> [<dir> ...]
// (the section flags drop Engine::load_directory, which safetensors.cpp also holds and which needs the whole engine)
// Every <dir> holds an llm.safetensors of the tiny4 geometry of tests/cvlm_cases.py (qasr.synth.write_cosyvoice_llm_safetensors); the
// program prints "accepted" or the refusal for each.  It walks the keys as CosyLlm::load_all does.
#include "qlm_weights.h"
#include <cstdio>
#include <cstdlib>

namespace qasr {          // a dry loader packs nothing: the image builder (dec_quant.hip) is not linked
size_t quant_q_bytes(int, int, int) { std::abort(); }
size_t quant_sb_bytes(int, int, int) { std::abort(); }
void quant_pack_launch(const QuantRaw&, uint32_t*, void*, hipStream_t) { std::abort(); }
}  // namespace qasr

using namespace qasr;

int main(int argc, char** argv) {
    const int H = 384, heads = 6, kv = 2, hd = 64, inter = 640, layers = 3, bits = 4, text_vocab = 1024, V = 13 + 8;
    for (int i = 1; i < argc; ++i) {
        try {
            SafeTensorsDir st(argv[i], "llm.safetensors");
            QlmLoader wl("cosyvoice llm", nullptr, true);
            wl.bf16(st, "text_embedding.weight", {text_vocab, H});
            wl.bf16(st, "speech_embedding.weight", {V, H});
            for (int l = 0; l < layers; ++l) {
                const std::string p = "layers." + std::to_string(l) + ".";
                QlmLayer L = qlm_load_layer(wl, st, p, {H, heads * hd, kv * hd, inter, bits}, QlmBias::BF16);
                for (QLin* q : {&L.qkv, &L.o, &L.gu, &L.down}) wl.pack(*q);
            }
            wl.bf16(st, "norm.weight", {H});
            QLin head = wl.qlin(st, {"speech_head"}, H, bits, QlmBias::NONE, 0, (V + 15) / 16 * 16);
            if (head.N != V) wl.refuse("speech_head holds " + std::to_string(head.N) + " rows");
            wl.refuse_unexpected(st);
            std::printf("%s: accepted\n", argv[i]);
        } catch (const WeightLoadError& e) {
            std::printf("%s: refused (%d): %s\n", argv[i], e.code, e.what());
        } catch (const std::exception& e) {
            std::printf("%s: not read: %s\n", argv[i], e.what());
        }
    }
    return 0;
}
