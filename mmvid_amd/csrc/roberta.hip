// RoBERTa-large, the frozen text encoder of `--fixed_language_model roberta-large` (utils/utils_train.py:194-222, train.py:274-290,
// test.py:85-86), around the kernels it shares with the CLIP tower: transformers' RobertaEmbeddings.forward (token ids -> position ids
// -> word + position + token_type rows -> LayerNorm), the post-LN RobertaLayer loop (RobertaSelfAttention / SelfOutput / Intermediate /
// Output) and utils/utils.py:53-59 mean_pooling.
//
//   embed_ln        ids [B,L] -> x [B*L,E] fp32 + bf16, key_len [B] (one wave per token row)
//   encoder         x = LN(x + Wo attn(Wqkv x)) ; x = LN(x + W2 gelu(W1 x)) per layer: mmvid_gemm_bf16 (act 2 = erf GELU),
//                   mmvid_attention_fwd_keylen, mmvid_layernorm_fwd.  Inference only, no allocation, no host sync.
//   mean_pool       [B,L,E] fp32 -> [B,E]: sum of the rows whose mask is non-zero / max(count, 1e-9)
#include "../../include/mmvid_hip.h"
#include "common.h"
#include "graphs.h"

namespace {

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

#define TRY(call)                   \
    do {                            \
        int rc__ = (call);          \
        if (rc__ != 0) return rc__; \
    } while (0)

constexpr int kMaxE = 1024;  // 16 values per lane

// One wave per token (b, i).  Position id (modeling_roberta.py create_position_ids_from_input_ids):
//   pad + cumsum(ids != pad)[i] for a real token, pad for a pad token.
// key_len[b] (written by the wave of i == 0) = number of non-zero mask entries (mask NULL: ids != pad), or -1 when they are not a
// prefix of the row.  Sums in the order word + position + token_type (RobertaEmbeddings: inputs_embeds + token_type_embeddings, then
// + position_embeddings: fp32 addition is commutative, so the two-term orders agree bit for bit; three terms are added as the model
// does), LayerNorm statistics in fp32 (two-pass: mean, then the centred sum of squares).
__global__ __launch_bounds__(256) void roberta_embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, int B,
                                                               int L, const float* __restrict__ word, int64_t vocab,
                                                               const float* __restrict__ pos, int64_t npos, const float* __restrict__ type0,
                                                               const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
                                                               int E, int64_t pad, float* __restrict__ x, bf16_t* __restrict__ xb,
                                                               int32_t* __restrict__ key_len) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * L) return;
    const int b = (int)(row / L), i = (int)(row - (int64_t)b * L);
    const int64_t* rid = ids + (int64_t)b * L;
    // count of real tokens in [0, i] (a wave-wide ballot over 64 positions at a time)
    int cnt = 0;
    for (int j0 = 0; j0 <= i; j0 += 64) {
        const int j = j0 + lane;
        const bool real = j <= i && rid[j] != pad;
        cnt += __popcll(__ballot(real));
    }
    if (i == 0) {  // key length and the prefix test of the whole row
        const int64_t* rm = mask ? mask + (int64_t)b * L : nullptr;
        int n = 0, holes = 0;
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            const bool live = j < L && (rm ? rm[j] != 0 : rid[j] != pad);
            const uint64_t bal = __ballot(live);
            const int c = __popcll(bal);
            // a prefix: every live position so far is at index < n + c, i.e. the ballot is the low c bits of this group and
            // no live position follows a dead one
            const uint64_t want = c == 64 ? ~0ull : ((1ull << c) - 1);
            holes |= (bal != want) || (c > 0 && n != j0);
            n += c;
        }
        if (lane == 0) key_len[b] = holes ? -1 : n;
    }
    const int64_t tok = rid[i];
    const int64_t t = (tok >= 0 && tok < vocab) ? tok : 0;
    int64_t p = tok != pad ? pad + cnt : pad;
    if (p >= npos) p = npos - 1;  // (beyond max_position_embeddings: the module's index error; never reached for L <= npos - pad - 1)
    const float* wr = word + t * E;
    const float* pr = pos + p * E;
    const int per = E >> 6;
    float v[kMaxE / 64];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxE / 64; ++k) {
        if (k < per) {
            const int c = k * 64 + lane;
            v[k] = (wr[c] + type0[c]) + pr[c];
            s += v[k];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)E;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxE / 64; ++k)
        if (k < per) {
            const float d = v[k] - mean;
            q += d * d;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = rsqrtf(q / (float)E + eps);
#pragma unroll
    for (int k = 0; k < kMaxE / 64; ++k)
        if (k < per) {
            const int c = k * 64 + lane;
            const float y = (v[k] - mean) * rstd * ln_w[c] + ln_b[c];
            x[row * E + c] = y;
            if (xb) xb[row * E + c] = f2bf(y);
        }
}

// One block per (sequence, 256 columns): fp32 sums of the rows whose mask is non-zero, in ascending row order; padded rows are
// skipped, never multiplied (their contents need not be finite).
__global__ __launch_bounds__(256) void roberta_mean_pool_kernel(const float* __restrict__ x, const int64_t* __restrict__ mask, int L,
                                                                int E, float* __restrict__ out) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= E) return;
    const int64_t* m = mask + (int64_t)b * L;
    const float* xr = x + (int64_t)b * L * E + c;
    float s = 0.f, n = 0.f;
    for (int l = 0; l < L; ++l)
        if (m[l] != 0) s += xr[(int64_t)l * E], n += 1.f;
    out[(int64_t)b * E + c] = s / fmaxf(n, 1e-9f);
}

struct Scratch {
    int64_t xb, qkv, o, t, x1, x1b, act, xa, total;
};
Scratch scratch_layout(const mmvid_postln_cfg_t& c) {
    const int64_t M = (int64_t)c.B * c.L;
    Scratch s;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        int64_t o = off;
        off += align256(bytes);
        return o;
    };
    s.xb = take(M * c.E * 2);
    s.qkv = take(M * 3 * c.E * 2);
    s.o = take(M * c.E * 2);
    s.t = take(M * c.E * 4);
    s.x1 = take(M * c.E * 4);
    s.x1b = take(M * c.E * 2);
    s.act = take(M * c.F * 2);
    s.xa = take(M * c.E * 4);
    s.total = off;
    return s;
}

int check_cfg(const mmvid_postln_cfg_t* c) {
    MMVID_REQUIRE(c, "postln_encoder: null config");
    MMVID_REQUIRE(c->B > 0 && c->L > 0 && c->layers > 0, "postln_encoder: bad B/L/layers");
    MMVID_REQUIRE(c->E == c->H * 64 && c->F % 8 == 0 && c->E <= kMaxE,
                  "postln_encoder: need E == 64*H <= %d and F %% 8 == 0 (E=%d H=%d F=%d)", kMaxE, c->E, c->H, c->F);
    return 0;
}

// Y = X W^T + b (+ residual) (act) with X [M,K] and W [N,K] row-major bf16
int linear(int64_t M, int N, int K, const void* X, const void* W, const float* bias, const float* residual, int act, float* out_f32,
           void* out_bf16, void* st) {
    return mmvid_gemm_bf16(0, 0, (int)M, N, K, X, K, W, K, 1, 0, 0, 0, 1, 1.0f, bias, residual, N, nullptr, nullptr, N, act, 0, out_f32,
                           out_bf16, N, nullptr, st);
}

int encoder_enqueue(const mmvid_postln_cfg_t* cfg, const mmvid_postln_layer_t* layers, const int32_t* key_len, const float* x_in,
                    const void* x_in_bf16, float* x_out, void* scratch, void* stream) {
    const mmvid_postln_cfg_t& c = *cfg;
    const int64_t M = (int64_t)c.B * c.L;
    const int E = c.E, F = c.F;
    const Scratch sc = scratch_layout(c);
    char* s = (char*)scratch;
    void *xb = s + sc.xb, *qkv = s + sc.qkv, *o = s + sc.o, *x1b = s + sc.x1b, *act = s + sc.act;
    float *t = (float*)(s + sc.t), *x1 = (float*)(s + sc.x1), *xa = (float*)(s + sc.xa);
    const float scale = 0.125f;  // head_dim^-0.5, head_dim = 64
    if (!x_in_bf16) TRY(mmvid_cast_f32_to_bf16(x_in, xb, M * E, stream));
    const float* x = x_in;
    const void* xin_b = x_in_bf16 ? x_in_bf16 : xb;
    for (int i = 0; i < c.layers; ++i) {
        const mmvid_postln_layer_t& ly = layers[i];
        float* xnext = i == c.layers - 1 ? x_out : xa;
        // RobertaSelfAttention (query | key | value packed as one [3E, E] weight) -> RobertaSelfOutput: LayerNorm(dense(ctx) + x)
        TRY(linear(M, 3 * E, E, xin_b, ly.qkv_w, ly.qkv_b, nullptr, 0, nullptr, qkv, stream));
        TRY(mmvid_attention_fwd_keylen(qkv, 3 * E, c.B, c.L, c.H, E, scale, key_len, o, E, nullptr, stream));
        TRY(linear(M, E, E, o, ly.out_w, ly.out_b, x, 0, t, nullptr, stream));
        TRY(mmvid_layernorm_fwd(t, E, M, E, ly.ln1_w, ly.ln1_b, c.ln_eps, x1b, x1, E, nullptr, nullptr, stream));
        // RobertaIntermediate (dense + erf GELU) -> RobertaOutput: LayerNorm(dense(h) + x1)
        TRY(linear(M, F, E, x1b, ly.fc_w, ly.fc_b, nullptr, 2, nullptr, act, stream));
        TRY(linear(M, E, F, act, ly.pj_w, ly.pj_b, x1, 0, t, nullptr, stream));
        TRY(mmvid_layernorm_fwd(t, E, M, E, ly.ln2_w, ly.ln2_b, c.ln_eps, xb, xnext, E, nullptr, nullptr, stream));
        x = xnext, xin_b = xb;
    }
    return MMVID_OK;
}

}  // namespace

extern "C" int mmvid_roberta_embed(const int64_t* ids, const int64_t* mask, int B, int L, const float* word, int64_t vocab,
                                   const float* pos, int64_t npos, const float* type0, const float* ln_w, const float* ln_b, float eps,
                                   int E, int64_t pad_idx, float* x_f32, void* x_bf16, int32_t* key_len, void* stream) {
    MMVID_REQUIRE(ids && word && pos && type0 && ln_w && ln_b && x_f32 && key_len, "roberta_embed: null pointer");
    MMVID_REQUIRE(B > 0 && L > 0 && E % 64 == 0 && E <= kMaxE, "roberta_embed: need B, L > 0 and E a multiple of 64 <= %d (E=%d)", kMaxE, E);
    MMVID_REQUIRE(vocab > 0 && pad_idx >= 0 && pad_idx < npos, "roberta_embed: bad vocab (%lld) / padding_idx (%lld) / positions (%lld)",
                  (long long)vocab, (long long)pad_idx, (long long)npos);
    MMVID_REQUIRE(L + pad_idx < npos, "roberta_embed: L = %d needs %lld position rows, the table has %lld", L, (long long)(L + pad_idx + 1),
                  (long long)npos);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * L;
    hipLaunchKernelGGL(roberta_embed_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ids, mask, B, L, word, vocab, pos, npos,
                       type0, ln_w, ln_b, eps, E, pad_idx, x_f32, (bf16_t*)x_bf16, key_len);
    MMVID_LAUNCH_CHECK("roberta_embed");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    if (cap == hipStreamCaptureStatusNone) {  // the prefix test: one read of key_len (under capture a bad row is left at -1)
        int32_t kl[256];
        for (int b0 = 0; b0 < B; b0 += 256) {
            const int n = B - b0 < 256 ? B - b0 : 256;
            if (hipMemcpyAsync(kl, key_len + b0, n * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess) {
                mmvid_set_error("roberta_embed: reading key_len back failed");
                return MMVID_ERR_HIP;
            }
            for (int k = 0; k < n; ++k)
                MMVID_REQUIRE(kl[k] >= 0, "roberta_embed: the attention mask of row %d is not a prefix (a pad before a real token)", b0 + k);
        }
    }
    return MMVID_OK;
}

extern "C" int mmvid_masked_mean_pool(const float* x, const int64_t* mask, int B, int L, int E, float* out, void* stream) {
    MMVID_REQUIRE(x && mask && out, "masked_mean_pool: null pointer");
    MMVID_REQUIRE(B >= 0 && L > 0 && E > 0, "masked_mean_pool: bad sizes B=%d L=%d E=%d", B, L, E);
    if (B == 0) return MMVID_OK;
    hipLaunchKernelGGL(roberta_mean_pool_kernel, dim3(cdiv(E, 256), B), dim3(256), 0, (hipStream_t)stream, x, mask, L, E, out);
    MMVID_LAUNCH_CHECK("masked_mean_pool");
    return MMVID_OK;
}

extern "C" int mmvid_postln_encoder_workspace(const mmvid_postln_cfg_t* cfg, int64_t* scratch_bytes) {
    TRY(check_cfg(cfg));
    if (scratch_bytes) *scratch_bytes = scratch_layout(*cfg).total;
    return MMVID_OK;
}

extern "C" int mmvid_postln_encoder_forward(const mmvid_postln_cfg_t* cfg, const mmvid_postln_layer_t* layers, const int32_t* key_len,
                                            const float* x_in, const void* x_in_bf16, float* x_out, void* scratch, void* stream) {
    TRY(check_cfg(cfg));
    MMVID_REQUIRE(layers && key_len && x_in && x_out && scratch, "postln_encoder_forward: null pointer");
    uint64_t k = mmvid_hash_bytes(cfg, sizeof(*cfg), 0xcbf29ce484222325ull ^ 7);
    k = mmvid_hash_bytes(layers, sizeof(mmvid_postln_layer_t) * (size_t)cfg->layers, k);
    for (const void* p : {(const void*)key_len, (const void*)x_in, x_in_bf16, (const void*)x_out, (const void*)scratch, (const void*)stream})
        k = mmvid_hash_ptr(p, k);
    return mmvid_run_cached(k, (hipStream_t)stream, [=](hipStream_t s) {
        return encoder_enqueue(cfg, layers, key_len, x_in, x_in_bf16, x_out, scratch, (void*)s);
    });
}
