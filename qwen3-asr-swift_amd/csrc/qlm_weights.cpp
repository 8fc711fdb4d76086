// qlm_weights.cpp -- the checked weight loader of the quantised speech LMs (qlm_weights.h).
#include "qlm_weights.h"
#include <algorithm>
#include <cstring>

namespace qasr {

static std::string shape_str(const std::vector<int64_t>& s) {
    std::string r = "[";
    for (size_t i = 0; i < s.size(); ++i) r += (i ? ", " : "") + std::to_string(s[i]);
    return r + "]";
}
static bool is_float(const SafeEntry& e) { return e.dtype == "F32" || e.dtype == "F16" || e.dtype == "BF16"; }

void QlmLoader::refuse(const std::string& what) const { throw WeightLoadError(QASR_ERR_INVALID, who_ + ": " + what); }

void* QlmLoader::upload(const void* src, size_t bytes) {
    auto buf = std::make_unique<DevBuf>();
    buf->alloc(bytes);
    device_bytes_ += buf->bytes;
    if (src) QASR_HIP(hipMemcpyAsync(buf->p, src, bytes, hipMemcpyHostToDevice, stream_));
    void* p = buf->p;
    bufs_.push_back(std::move(buf));
    if (src) QASR_HIP(hipStreamSynchronize(stream_));     // src may be a temporary
    return p;
}

const SafeEntry& QlmLoader::need(const SafeTensorsDir& st, const std::string& key) {
    auto it = st.entries.find(key);
    if (it == st.entries.end()) throw WeightLoadError(QASR_ERR_IO, who_ + ": missing tensor " + key);
    seen_.insert(key);
    return it->second;
}

void QlmLoader::refuse_unexpected(const SafeTensorsDir& st) const {
    for (const auto& kv : st.entries)
        if (!seen_.count(kv.first)) refuse("unexpected tensor " + kv.first);
}

const bf16_t* QlmLoader::bf16(const SafeTensorsDir& st, const std::string& key, std::vector<int64_t> shape) {
    const SafeEntry& e = need(st, key);
    if (e.shape != shape) refuse("tensor " + key + " has shape " + shape_str(e.shape) + ", expected " + shape_str(shape));
    if (!is_float(e)) refuse("tensor " + key + " has dtype " + e.dtype + " (F32 / F16 / BF16)");
    if (dry_) return nullptr;
    param_bytes_ += e.bytes;
    if (e.dtype == "BF16") return (const bf16_t*)upload(e.data, e.bytes);
    std::vector<bf16_t> h(e.numel());
    for (size_t i = 0; i < h.size(); ++i) h[i] = f32_to_bf16_host(safe_elem_f32(e, i));
    return (const bf16_t*)upload(h.data(), h.size() * sizeof(bf16_t));
}

QLin QlmLoader::qlin(const SafeTensorsDir& st, const std::vector<std::string>& stems, int K, int bits, QlmBias bias, int interleave,
                     int pad_to) {
    const int wrow = K * bits / 32, G = K / 64;
    struct Part { const SafeEntry *w, *s, *b, *lb; int N; };
    std::vector<Part> parts;
    std::string sdtype;
    for (const auto& stem : stems) {
        const SafeEntry& w = need(st, stem + ".weight");
        if (is_float(w))
            refuse("tensor " + stem + ".weight is float (" + w.dtype + "): a float (unquantised) checkpoint is not served, only MLX affine 4 / 8 bit");
        if (w.dtype != "U32" || w.shape.size() != 2 || w.shape[1] != wrow)
            refuse("tensor " + stem + ".weight has dtype " + w.dtype + " shape " + shape_str(w.shape) + ", expected U32 [N, " + std::to_string(wrow) +
                   "] (bits / width mismatch)");
        const SafeEntry &s = need(st, stem + ".scales"), &b = need(st, stem + ".biases");
        for (const SafeEntry* t : {&s, &b}) {
            if (t->shape != std::vector<int64_t>{w.shape[0], (int64_t)G})
                refuse(stem + " scales / biases have shape " + shape_str(t->shape) + ", expected " + shape_str({w.shape[0], (int64_t)G}));
            if (!is_float(*t)) refuse(stem + " scales / biases have dtype " + t->dtype);
        }
        if (s.dtype != b.dtype || (!sdtype.empty() && sdtype != s.dtype)) refuse(stem + " scales / biases differ in dtype");
        sdtype = s.dtype;
        const SafeEntry* lb = nullptr;
        if (bias != QlmBias::NONE) {
            lb = &need(st, stem + ".bias");
            if (lb->shape != std::vector<int64_t>{w.shape[0]} || !is_float(*lb))
                refuse("tensor " + stem + ".bias has shape " + shape_str(lb->shape) + " dtype " + lb->dtype + ", expected float [" +
                       std::to_string(w.shape[0]) + "]");
        }
        parts.push_back({&w, &s, &b, lb, (int)w.shape[0]});
        if (!dry_) param_bytes_ += w.bytes + s.bytes + b.bytes + (lb ? lb->bytes : 0);
    }
    std::vector<std::pair<int, int>> order;            // (part, row): the order of source rows
    if (interleave) {
        if (parts.size() != 2 || parts[0].N != parts[1].N || parts[0].N % interleave) refuse(stems[0] + ": gate / up row counts do not interleave");
        for (int blk = 0; blk < parts[0].N / interleave; ++blk)
            for (int pi = 0; pi < 2; ++pi)
                for (int r = 0; r < interleave; ++r) order.push_back({pi, blk * interleave + r});
    } else {
        for (size_t pi = 0; pi < parts.size(); ++pi)
            for (int r = 0; r < parts[pi].N; ++r) order.push_back({(int)pi, r});
    }
    const int Nsrc = (int)order.size(), N = std::max(Nsrc, pad_to);
    QLin L;
    L.N = Nsrc; L.K = K;
    if (dry_) return L;
    const bool keep_bf16 = sdtype == "BF16";
    const size_t sel = keep_bf16 ? 2 : 4;
    std::vector<uint32_t> hw((size_t)N * wrow, 0u);
    std::vector<uint8_t> hs((size_t)N * G * sel, 0), hb((size_t)N * G * sel, 0);
    std::vector<float> hl(bias != QlmBias::NONE ? N : 0, 0.0f);
    for (int n = 0; n < Nsrc; ++n) {
        const Part& pt = parts[order[n].first];
        const int r = order[n].second;
        std::memcpy(&hw[(size_t)n * wrow], pt.w->data + (size_t)r * wrow * 4, (size_t)wrow * 4);
        if (keep_bf16 || sdtype == "F32") {
            std::memcpy(&hs[(size_t)n * G * sel], pt.s->data + (size_t)r * G * sel, G * sel);
            std::memcpy(&hb[(size_t)n * G * sel], pt.b->data + (size_t)r * G * sel, G * sel);
        } else {
            for (int g = 0; g < G; ++g) {
                reinterpret_cast<float*>(hs.data())[(size_t)n * G + g] = safe_elem_f32(*pt.s, (size_t)r * G + g);
                reinterpret_cast<float*>(hb.data())[(size_t)n * G + g] = safe_elem_f32(*pt.b, (size_t)r * G + g);
            }
        }
        if (pt.lb) {
            const float v = safe_elem_f32(*pt.lb, r);
            hl[n] = bias == QlmBias::BF16 ? bf16_to_f32_host(f32_to_bf16_host(v)) : v;
        }
    }
    QuantRaw raw;
    raw.wq = (const uint32_t*)upload(hw.data(), hw.size() * 4);
    raw.scales = upload(hs.data(), hs.size());
    raw.biases = upload(hb.data(), hb.size());
    raw.sb_f32 = keep_bf16 ? 0 : 1; raw.N = N; raw.K = K; raw.bits = bits;
    L.img.raw = raw; L.img.bits = bits; L.img.sb_f32 = raw.sb_f32;
    if (bias != QlmBias::NONE) L.bias = (const float*)upload(hl.data(), hl.size() * 4);
    return L;
}

void QlmLoader::pack(QLin& q) {
    if (dry_) return;
    const QuantRaw& raw = q.img.raw;
    uint32_t* qp = (uint32_t*)upload(nullptr, quant_q_bytes(raw.N, raw.K, raw.bits));
    void* sb = upload(nullptr, quant_sb_bytes(raw.N, raw.K, raw.sb_f32));
    quant_pack_launch(raw, qp, sb, stream_);
    QASR_HIP(hipGetLastError());
    q.img.qp = qp; q.img.sb = sb;
}

QlmLayer qlm_load_layer(QlmLoader& wl, const SafeTensorsDir& st, const std::string& p, const QlmLayerGeom& g, QlmBias qkv_bias) {
    QlmLayer L;
    L.qkv = wl.qlin(st, {p + "self_attn.q_proj", p + "self_attn.k_proj", p + "self_attn.v_proj"}, g.H, g.bits, qkv_bias);
    if (L.qkv.N != g.nq + 2 * g.nkv)
        wl.refuse(p + "self_attn q/k/v_proj hold " + std::to_string(L.qkv.N) + " rows, expected " + std::to_string(g.nq + 2 * g.nkv));
    L.o = wl.qlin(st, {p + "self_attn.o_proj"}, g.nq, g.bits);
    L.gu = wl.qlin(st, {p + "mlp.gate_proj", p + "mlp.up_proj"}, g.H, g.bits, QlmBias::NONE, 16);
    L.down = wl.qlin(st, {p + "mlp.down_proj"}, g.I, g.bits);
    if (L.o.N != g.H || L.gu.N != 2 * g.I || L.down.N != g.H) wl.refuse(p + " o_proj / mlp row counts do not match the geometry");
    L.ln1 = wl.bf16(st, p + "input_layernorm.weight", {g.H});
    L.ln2 = wl.bf16(st, p + "post_attention_layernorm.weight", {g.H});
    return L;
}

}  // namespace qasr
