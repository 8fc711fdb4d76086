// api_vloc.cpp -- extern "C" boundary of VoxCPM2's local networks (include/qasr.h, qasr_vloc_*).  Exceptions never cross it.
#include "api_guard.h"
#include "loc_voxcpm.h"
#include "voc_cosyvoice.h"
#include <memory>

struct qasr_vloc {
    std::unique_ptr<qasr::LocVoxcpm> impl;
    mutable std::string last_error;
};
static std::string& error_slot(const qasr_vloc* h) { return h ? h->last_error : create_error<qasr_vloc>(); }

using namespace qasr;

static const char* const WHO = "VoxCPM2 local networks";

// NOT_LOADED comes before every other refusal
static int ready(qasr_vloc* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (!h->impl->loaded()) return fail(h, QASR_ERR_NOT_LOADED, std::string(WHO) + ": model unloaded");
    return QASR_OK;
}

static int null_argument(qasr_vloc* h) { return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": null argument"); }

static int over(qasr_vloc* h, size_t B) {
    return fail(h, QASR_ERR_CAPACITY, std::string(WHO) + ": B = " + std::to_string(B) + " exceeds max_seqs = " + std::to_string(h->impl->max_seqs()));
}

// the configuration, then every key, shape and dtype: host work only
static int read_checkpoint(const char* model_dir, VlocConfig& cfg, VlocWeights& w) {
    if (!model_dir) return fail<qasr_vloc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": model_dir is NULL");
    try {
        cfg = vloc_read_config(model_dir, WHO);
        w = vloc_load_weights(model_dir, WHO, cfg);
    } catch (const WeightLoadError& ex) { return fail<qasr_vloc>(nullptr, ex.code, ex.what()); }
    catch (const std::invalid_argument& ex) { return fail<qasr_vloc>(nullptr, QASR_ERR_INVALID, ex.what()); }
    catch (const std::exception& ex) { return fail<qasr_vloc>(nullptr, QASR_ERR_IO, ex.what()); }
    return QASR_OK;
}

extern "C" {

int qasr_vloc_check(const char* model_dir, qasr_vloc_geometry* g) {
    VlocConfig cfg;
    VlocWeights w;
    if (const int rc = read_checkpoint(model_dir, cfg, w)) return rc;
    if (g) {
        g->patch_size = cfg.patch_size; g->feat_dim = cfg.feat_dim; g->lm_hidden = cfg.lm_hidden; g->enc_hidden = cfg.enc.hidden;
        g->dit_hidden = cfg.dit.hidden; g->enc_layers = cfg.enc.layers; g->dit_layers = cfg.dit.layers; g->mu_dim = cfg.mu_dim();
        g->kv_heads = cfg.kv_heads; g->stored_bytes = w.f.disk_bytes;
    }
    return QASR_OK;
}

int qasr_vloc_create(int device, const char* model_dir, size_t max_seqs, qasr_engine* order_with, qasr_vloc** out) {
    if (!out) return QASR_ERR_INVALID;
    *out = nullptr;
    if (max_seqs == 0) max_seqs = (size_t)VL_DEFAULT_SEQS;
    if (max_seqs > (size_t)VL_MAX_SEQS) return fail<qasr_vloc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": max_seqs in 1..1024 (0 = 32)");
    if (order_with && (!order_with->impl || order_with->impl->config().device != device))
        return fail<qasr_vloc>(nullptr, QASR_ERR_INVALID, std::string(WHO) + ": order_with must be an engine on the same device");
    VlocConfig cfg;
    VlocWeights w;
    if (const int rc = read_checkpoint(model_dir, cfg, w)) return rc;
    return guarded_create(out, QASR_ERR_INVALID, [&](qasr_vloc* h) {
        h->impl = std::make_unique<LocVoxcpm>(device, cfg, w, (long)max_seqs, order_with ? order_with->impl->stream() : nullptr);
    });
}

void qasr_vloc_destroy(qasr_vloc* h) { delete h; }
const char* qasr_vloc_last_error(const qasr_vloc* h) { return error_slot(h).c_str(); }
int qasr_vloc_is_loaded(const qasr_vloc* h) { return h && h->impl && h->impl->loaded() ? 1 : 0; }
int qasr_vloc_unload(qasr_vloc* h) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    return guarded(h, [&] { h->impl->unload(); });
}
size_t qasr_vloc_memory_footprint(const qasr_vloc* h) { return h && h->impl ? h->impl->footprint() : 0; }
int qasr_vloc_patch_size(const qasr_vloc* h) { return h && h->impl ? h->impl->config().patch_size : 0; }
int qasr_vloc_feat_dim(const qasr_vloc* h) { return h && h->impl ? h->impl->config().feat_dim : 0; }
int qasr_vloc_lm_hidden(const qasr_vloc* h) { return h && h->impl ? h->impl->config().lm_hidden : 0; }
int qasr_vloc_mu_dim(const qasr_vloc* h) { return h && h->impl ? h->impl->config().mu_dim() : 0; }
int qasr_vloc_hidden(const qasr_vloc* h, int which) { return h && h->impl ? (which ? h->impl->config().dit.hidden : h->impl->config().enc.hidden) : 0; }
int qasr_vloc_depth(const qasr_vloc* h, int which) { return h && h->impl ? (which ? h->impl->config().dit.layers : h->impl->config().enc.layers) : 0; }
size_t qasr_vloc_max_seqs(const qasr_vloc* h) { return h && h->impl ? (size_t)h->impl->max_seqs() : 0; }

int qasr_vloc_schedule(int n_steps, float* t) {
    if (!t || n_steps < 1 || n_steps > VL_MAX_STEPS) return QASR_ERR_INVALID;
    vloc_schedule(n_steps, t);
    return QASR_OK;
}

int qasr_vloc_zero_steps(int n_steps) { return n_steps < 1 ? 0 : vloc_zero_steps(n_steps); }

int qasr_vloc_rope_table(const char* model_dir, int head_dim, int n_pos, float* cos, float* sin) {
    if (!model_dir || !cos || !sin || head_dim < 2 || head_dim % 2 || n_pos < 1) return QASR_ERR_INVALID;
    try {
        VlocConfig cfg = vloc_read_config(model_dir, WHO);
        vloc_rope_table(cfg, head_dim, n_pos, cos, sin);
    } catch (const std::exception& ex) { return fail<qasr_vloc>(nullptr, QASR_ERR_INVALID, ex.what()); }
    return QASR_OK;
}

int qasr_vloc_encode(qasr_vloc* h, const float* feats, size_t n, float* cls, float* embed) {
    if (const int rc = ready(h)) return rc;
    if (n == 0) return QASR_OK;
    if (!feats || (!cls && !embed)) return null_argument(h);
    return guarded(h, [&] { h->impl->encode(feats, (long)n, cls, embed); });
}

int qasr_vloc_mu(qasr_vloc* h, const float* lm_hidden, const float* res_hidden, size_t B, float* mu) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!lm_hidden || !res_hidden || !mu) return null_argument(h);
    if (B > (size_t)h->impl->max_seqs()) return over(h, B);
    return guarded(h, [&] { h->impl->mu(lm_hidden, res_hidden, (long)B, mu); });
}

int qasr_vloc_velocity(qasr_vloc* h, const float* x, const float* mu, const float* cond, size_t B, float t, float* v) {
    if (const int rc = ready(h)) return rc;
    if (B == 0) return QASR_OK;
    if (!x || !mu || !cond || !v) return null_argument(h);
    if (B > (size_t)h->impl->max_seqs()) return over(h, B);
    return guarded(h, [&] { h->impl->velocity(x, mu, cond, (long)B, t, v); });
}

int qasr_vloc_solve(qasr_vloc* h, const float* mu, const float* cond, const float* z, size_t B, int n_steps, float cfg, float* x_out, float* v_out) {
    if (const int rc = ready(h)) return rc;
    if (n_steps < 1 || n_steps > VL_MAX_STEPS) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": n_steps in 1..64");
    if (B == 0) return QASR_OK;
    if (!mu || !cond || !z || !x_out) return null_argument(h);
    if (B > (size_t)h->impl->max_seqs()) return over(h, B);
    return guarded(h, [&] { h->impl->solve(mu, cond, z, (long)B, n_steps, cfg, x_out, v_out); });
}

int qasr_vloc_sample(qasr_vloc* h, const float* mu, const float* cond, size_t B, int n_steps, float cfg, float temperature, uint64_t seed,
                     const uint64_t* row_index, float* z_out, float* x_out) {
    if (const int rc = ready(h)) return rc;
    if (n_steps < 1 || n_steps > VL_MAX_STEPS) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": n_steps in 1..64");
    if (B == 0) return QASR_OK;
    if (!mu || !cond || !x_out) return null_argument(h);
    if (B > (size_t)h->impl->max_seqs()) return over(h, B);
    // value i of row b = temperature x the normal of draw row_index[b] n + i of the stream `seed` (voc_cosyvoice.h), n = P feat_dim
    const size_t n = (size_t)h->impl->config().patch_size * h->impl->config().feat_dim;
    return guarded(h, [&] {
        std::vector<float> z(B * n);
        for (size_t b = 0; b < B; ++b)
            for (size_t i = 0; i < n; ++i) z[b * n + i] = temperature * hift_normal(hift_draw(seed, (row_index ? row_index[b] : b) * n + i));
        if (z_out) std::memcpy(z_out, z.data(), z.size() * sizeof(float));
        h->impl->solve(mu, cond, z.data(), (long)B, n_steps, cfg, x_out, nullptr);
    });
}

int qasr_vloc_stack(qasr_vloc* h, int which, const float* x, size_t n_seq, int S, int n_layers, float* out) {
    if (const int rc = ready(h)) return rc;
    if (which != 0 && which != 1) return fail(h, QASR_ERR_INVALID, std::string(WHO) + ": which is 0 (LocEnc) or 1 (LocDiT)");
    if (!x || !out) return null_argument(h);
    if (n_seq == 0) return QASR_OK;
    if (n_seq > 2 * (size_t)h->impl->max_seqs()) return over(h, n_seq);
    return guarded(h, [&] { h->impl->stack(which, x, (long)n_seq, S, n_layers, out); });
}

int qasr_vloc_timing(const qasr_vloc* h, float* ms) {
    if (!h || !h->impl) return QASR_ERR_INVALID;
    if (ms) std::memcpy(ms, h->impl->timing(), VL_TIMING * sizeof(float));
    return QASR_OK;
}

}  // extern "C"
