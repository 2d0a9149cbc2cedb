// The parts of OpenAI's CLIP around the two towers (mmvid_pytorch/transformers/clip_model.py:273-296 VisualTransformer.forward,
// 399-414 CLIP.encode_text, 416-432 CLIP.forward) and the frame preprocessing of utils/utils.py:62-85 clip_similarity.
// The towers themselves are mmvid_tower_forward (tower.hip), the patch embedding is mmvid_gemm_bf16 (gemm.hip).
//
//   patchify        frames [N,3,S,S] fp32 -> (nearest resize to R, (x - mean) / std) -> bf16 patch matrix [N*G*G, Kp]
//                   (Kp = 3*P*P rounded up to a multiple of 64, zero pad columns: the patch GEMM's K never has a ragged tile)
//   image_assemble  patch features [N*G*G, E] fp32 -> [class | patches] + positional_embedding -> ln_pre -> [N, G*G+1, E] fp32
//   text_embed      ids [B,L] -> token_embedding rows + positional_embedding [B,L,E] fp32, and argmax(ids) per row (first maximum)
//   pool_project    one row per sequence -> ln_post / ln_final -> @ proj [E,D] -> (optional) L2 normalisation -> [B,D] fp32
//   pair_scores     out[b*T+t] = <img[b*T+t], txt[b]> (clip_similarity's per-frame dot product)
// All wave64; LayerNorm statistics and every dot product in fp32.
#include "common.h"
#include "../../include/mmvid_hip.h"

namespace {

// OpenAI CLIP's image normalisation (utils/utils.py:69-70) as the fp32 values torch.tensor([...]) holds
__constant__ float kMean[3] = {0x1.ed0274p-2f, 0x1.d4d0bcp-2f, 0x1.a201fep-2f};
__constant__ float kStd[3] = {0x1.1313a0p-2f, 0x1.0b92e8p-2f, 0x1.1a6550p-2f};

// One thread per 8 consecutive kx of one (frame, patch, channel, ky): column order (c, ky, kx) = conv1.weight.reshape(E, 3*P*P).
// resize: ATen's `nearest` rule, src = min(floor(dst * scale), S - 1) with scale = (float)S / R in fp32 (identity when S == R).
__global__ __launch_bounds__(256) void clip_patchify_kernel(const float* __restrict__ x, int64_t total, int S, int R, int P, int G,
                                                            int normalize, float scale, bf16_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cols8 = 3 * P * P / 8;
    const int64_t row = t / cols8;
    const int col = (int)(t - row * cols8) * 8;
    const int c = col / (P * P), rem = col - c * P * P;
    const int ky = rem / P, kx0 = rem - ky * P;
    const int64_t n = row / (G * G);
    const int p = (int)(row - n * G * G), py = p / G, px = p - py * G;
    const int y = py * P + ky, x0 = px * P + kx0;
    const int sy = normalize ? min((int)floorf((float)y * scale), S - 1) : y;
    const float* src = x + ((n * 3 + c) * S + sy) * (int64_t)S;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int sx = normalize ? min((int)floorf((float)(x0 + j) * scale), S - 1) : x0 + j;
        v[j] = src[sx];
        if (normalize) v[j] = __fdiv_rn(__fsub_rn(v[j], kMean[c]), kStd[c]);
    }
    uint4 o;
    o.x = pack_bf2(v[0], v[1]), o.y = pack_bf2(v[2], v[3]), o.z = pack_bf2(v[4], v[5]), o.w = pack_bf2(v[6], v[7]);
    *reinterpret_cast<uint4*>(out + row * (3 * P * P) + col) = o;
}

// Any patch size: rows of Kp = 3*P*P rounded up to a multiple of 64 columns, columns [3*P*P, Kp) +0.0.  One thread per 8 consecutive
// columns of one row (one 16-byte store; Kp % 8 == 0, so a store never crosses a row): the first column is decoded into (c, ky, kx)
// by division, the next seven by carrying (kx -> ky -> c), and c >= 3 marks a pad column.  Each value is clip_patchify_kernel's
// expression, so where both kernels apply they store the same bytes.
__global__ __launch_bounds__(256) void clip_patchify_padded_kernel(const float* __restrict__ x, int64_t total, int S, int R, int P, int G,
                                                                   int Kp, int normalize, float scale, bf16_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cols8 = Kp / 8;
    const int64_t row = t / cols8;
    const int col = (int)(t - row * cols8) * 8;
    int c = col / (P * P);
    const int rem = col - c * P * P;
    int ky = rem / P, kx = rem - ky * P;
    const int64_t n = row / (G * G);
    const int p = (int)(row - n * G * G), py = p / G, px = p - py * G;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = 0.f;
        if (c < 3) {
            const int y = py * P + ky, xx = px * P + kx;
            const int sy = normalize ? min((int)floorf((float)y * scale), S - 1) : y;
            const int sx = normalize ? min((int)floorf((float)xx * scale), S - 1) : xx;
            v[j] = x[((n * 3 + c) * S + sy) * (int64_t)S + sx];
            if (normalize) v[j] = __fdiv_rn(__fsub_rn(v[j], kMean[c]), kStd[c]);
        }
        if (++kx == P) {
            kx = 0;
            if (++ky == P) ky = 0, ++c;
        }
    }
    uint4 o;
    o.x = pack_bf2(v[0], v[1]), o.y = pack_bf2(v[2], v[3]), o.z = pack_bf2(v[4], v[5]), o.w = pack_bf2(v[6], v[7]);
    *reinterpret_cast<uint4*>(out + row * Kp + col) = o;
}

// LayerNorm of NV float4 per lane (E = 256 * NV) held by one wave; y = (v - mean) * rstd * w + b
template <int NV>
__device__ __forceinline__ void wave_layernorm(float4 (&v)[NV], int lane, const float* __restrict__ w, const float* __restrict__ b,
                                               float eps, int E) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + bb * bb) + (c * c + d * d);
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float4 ww = reinterpret_cast<const float4*>(w)[lane + 64 * i], bv = reinterpret_cast<const float4*>(b)[lane + 64 * i];
        v[i] = make_float4((v[i].x - mean) * rstd * ww.x + bv.x, (v[i].y - mean) * rstd * ww.y + bv.y,
                           (v[i].z - mean) * rstd * ww.z + bv.z, (v[i].w - mean) * rstd * ww.w + bv.w);
    }
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// one wave per output row (n, t): t == 0 the class embedding, else patch t - 1; + pos[t]; ln_pre
template <int NV>
__global__ __launch_bounds__(256) void clip_image_assemble_kernel(const float* __restrict__ feat, const float* __restrict__ cls,
                                                                  const float* __restrict__ pos, const float* __restrict__ w,
                                                                  const float* __restrict__ b, float eps, int64_t rows, int T,
                                                                  float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    constexpr int E = 256 * NV;
    const int lane = threadIdx.x & 63;
    const int64_t n = row / T;
    const int t = (int)(row - n * T);
    const float4* src = reinterpret_cast<const float4*>(t == 0 ? cls : feat + (n * (T - 1) + t - 1) * E);
    const float4* pp = reinterpret_cast<const float4*>(pos + (int64_t)t * E);
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = add4(src[lane + 64 * i], pp[lane + 64 * i]);
    wave_layernorm<NV>(v, lane, w, b, eps, E);
    float4* dst = reinterpret_cast<float4*>(out + row * E);
#pragma unroll
    for (int i = 0; i < NV; ++i) dst[lane + 64 * i] = v[i];
}

// one wave per (b, l) row: token_embedding[id] + pos[l] (an id outside [0, vocab) reads row 0).  The wave of l == 0 also writes
// pool[b] = argmax over the row's ids, first maximum (torch.argmax), scanning all L ids.
template <int NV>
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const int64_t* __restrict__ ids, int64_t rows, int L,
                                                              const float* __restrict__ table, int64_t vocab,
                                                              const float* __restrict__ pos, float* __restrict__ out,
                                                              int32_t* __restrict__ pool) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    constexpr int E = 256 * NV;
    const int lane = threadIdx.x & 63;
    const int64_t bi = row / L;
    const int l = (int)(row - bi * L);
    int64_t id = ids[row];
    if (id < 0 || id >= vocab) id = 0;
    const float4* src = reinterpret_cast<const float4*>(table + id * E);
    const float4* pp = reinterpret_cast<const float4*>(pos + (int64_t)l * E);
    float4* dst = reinterpret_cast<float4*>(out + row * E);
#pragma unroll
    for (int i = 0; i < NV; ++i) dst[lane + 64 * i] = add4(src[lane + 64 * i], pp[lane + 64 * i]);
    if (l != 0 || !pool) return;
    const int64_t* r = ids + bi * L;
    int64_t best = INT64_MIN;
    int at = L;  // lanes without an id never win
    for (int j = lane; j < L; j += 64) {
        const int64_t v = r[j];
        if (v > best) best = v, at = j;  // ascending j: strict > keeps the first maximum
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
    }
    if (lane == 0) pool[bi] = at;
}

// Four sequences per block (one wave each): LayerNorm of the pooled row into LDS, then every thread owns output columns
// d = tid + 256 j (j < 4, D <= 1024) of all four sequences: y[s][d] = sum_k h[s][k] proj[k][d] (fmaf, k ascending).
constexpr int PP_SEQ = 4;
template <int NV>
__global__ __launch_bounds__(256) void clip_pool_project_kernel(const float* __restrict__ x, int B, int L, const int32_t* __restrict__ rows,
                                                                const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                                const float* __restrict__ proj, int D, int l2norm, float* __restrict__ out) {
    constexpr int E = 256 * NV;
    __shared__ float4 h[PP_SEQ][E / 4];
    __shared__ float red[4][PP_SEQ];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s0 = blockIdx.x * PP_SEQ;
    {
        const int s = s0 + wave;
        float4 v[NV];
        if (s < B) {
            int r = rows ? rows[s] : 0;
            r = min(max(r, 0), L - 1);
            const float4* src = reinterpret_cast<const float4*>(x + ((int64_t)s * L + r) * E);
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = src[lane + 64 * i];
            wave_layernorm<NV>(v, lane, w, b, eps, E);
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) h[wave][lane + 64 * i] = v[i];
    }
    __syncthreads();
    const float* hs = reinterpret_cast<const float*>(h);
    float acc[4][PP_SEQ];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < PP_SEQ; ++s) acc[j][s] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = threadIdx.x + 256 * j;
        if (d >= D) break;
        for (int k = 0; k < E; ++k) {
            const float pk = proj[(int64_t)k * D + d];
#pragma unroll
            for (int s = 0; s < PP_SEQ; ++s) acc[j][s] = fmaf(hs[s * E + k], pk, acc[j][s]);
        }
    }
    float scale[PP_SEQ];
#pragma unroll
    for (int s = 0; s < PP_SEQ; ++s) scale[s] = 1.f;
    if (l2norm) {
#pragma unroll
        for (int s = 0; s < PP_SEQ; ++s) {
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) q += acc[j][s] * acc[j][s];  // (zero for columns this thread does not own)
            q = wave_sum(q);
            if (lane == 0) red[wave][s] = q;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PP_SEQ; ++s) scale[s] = 1.f / sqrtf((red[0][s] + red[1][s]) + (red[2][s] + red[3][s]));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = threadIdx.x + 256 * j;
        if (d >= D) break;
#pragma unroll
        for (int s = 0; s < PP_SEQ; ++s)
            if (s0 + s < B) out[(int64_t)(s0 + s) * D + d] = l2norm ? acc[j][s] * scale[s] : acc[j][s];
    }
}

// one wave per frame
__global__ __launch_bounds__(256) void clip_pair_scores_kernel(const float* __restrict__ img, const float* __restrict__ txt, int64_t BT,
                                                               int T, int D, float* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= BT) return;
    const int lane = threadIdx.x & 63;
    const float* a = img + f * D;
    const float* t = txt + (f / T) * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = fmaf(a[k], t[k], s);
    s = wave_sum(s);
    if (lane == 0) out[f] = s;
}

int check_width(int E, const char* what) {
    MMVID_REQUIRE(E > 0 && E % 256 == 0 && E <= 1024, "%s: width %d must be a multiple of 256, at most 1024", what, E);
    return 0;
}

}  // namespace

extern "C" int mmvid_clip_patchify(const float* frames, int N, int S, int R, int P, int normalize, void* out_bf16, void* stream) {
    MMVID_REQUIRE(frames && out_bf16, "clip_patchify: null pointer");
    MMVID_REQUIRE(N > 0 && S > 0 && P > 0 && P <= 16384 && R > 0 && R % P == 0, "clip_patchify: bad sizes N=%d S=%d R=%d P=%d "
                  "(P at most 16384, dividing R)", N, S, R, P);
    MMVID_REQUIRE(normalize || S == R, "clip_patchify: normalize=0 takes frames already at the input resolution (S=%d, R=%d)", S, R);
    const int G = R / P;
    const float scale = (float)S / (float)R;
    if (P % 8 == 0) {  // 3*P*P is a multiple of 64: no pad columns
        const int64_t total = (int64_t)N * G * G * (3 * P * P / 8);
        hipLaunchKernelGGL(clip_patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, total,
                           S, R, P, G, normalize, scale, (bf16_t*)out_bf16);
    } else {
        const int Kp = (3 * P * P + 63) / 64 * 64;
        const int64_t total = (int64_t)N * G * G * (Kp / 8);
        hipLaunchKernelGGL(clip_patchify_padded_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames,
                           total, S, R, P, G, Kp, normalize, scale, (bf16_t*)out_bf16);
    }
    MMVID_LAUNCH_CHECK("clip_patchify");
    return MMVID_OK;
}

#define CLIP_NV_DISPATCH(E, KERNEL, GRID, STREAM, ...)                                                              \
    switch ((E) / 256) {                                                                                            \
        case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(256), 0, (hipStream_t)(STREAM), __VA_ARGS__); break;       \
        case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(256), 0, (hipStream_t)(STREAM), __VA_ARGS__); break;       \
        case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(256), 0, (hipStream_t)(STREAM), __VA_ARGS__); break;       \
        default: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(256), 0, (hipStream_t)(STREAM), __VA_ARGS__); break;      \
    }

extern "C" int mmvid_clip_image_assemble(const float* patch_feat, const float* class_emb, const float* pos, const float* ln_w,
                                         const float* ln_b, float eps, int N, int T, int E, float* out, void* stream) {
    MMVID_REQUIRE(patch_feat && class_emb && pos && ln_w && ln_b && out, "clip_image_assemble: null pointer");
    MMVID_REQUIRE(N > 0 && T > 1, "clip_image_assemble: bad sizes N=%d T=%d", N, T);
    if (check_width(E, "clip_image_assemble")) return MMVID_ERR_ARG;
    const int64_t rows = (int64_t)N * T;
    CLIP_NV_DISPATCH(E, clip_image_assemble_kernel, dim3((unsigned)((rows + 3) / 4)), stream, patch_feat, class_emb, pos, ln_w, ln_b, eps,
                     rows, T, out);
    MMVID_LAUNCH_CHECK("clip_image_assemble");
    return MMVID_OK;
}

extern "C" int mmvid_clip_text_embed(const int64_t* ids, int B, int L, const float* table, int64_t vocab, const float* pos, int E,
                                     float* out, int32_t* pool_idx, void* stream) {
    MMVID_REQUIRE(ids && table && pos && out, "clip_text_embed: null pointer");
    MMVID_REQUIRE(B > 0 && L > 0 && vocab > 0, "clip_text_embed: bad sizes B=%d L=%d", B, L);
    if (check_width(E, "clip_text_embed")) return MMVID_ERR_ARG;
    const int64_t rows = (int64_t)B * L;
    CLIP_NV_DISPATCH(E, clip_text_embed_kernel, dim3((unsigned)((rows + 3) / 4)), stream, ids, rows, L, table, vocab, pos, out, pool_idx);
    MMVID_LAUNCH_CHECK("clip_text_embed");
    return MMVID_OK;
}

extern "C" int mmvid_clip_pool_project(const float* x, int B, int L, int E, const int32_t* rows, const float* ln_w, const float* ln_b,
                                       float eps, const float* proj, int D, int l2norm, float* out, void* stream) {
    MMVID_REQUIRE(x && ln_w && ln_b && proj && out, "clip_pool_project: null pointer");
    MMVID_REQUIRE(B > 0 && L > 0 && D > 0 && D <= 1024, "clip_pool_project: bad sizes B=%d L=%d D=%d (D <= 1024)", B, L, D);
    if (check_width(E, "clip_pool_project")) return MMVID_ERR_ARG;
    CLIP_NV_DISPATCH(E, clip_pool_project_kernel, dim3((unsigned)((B + PP_SEQ - 1) / PP_SEQ)), stream, x, B, L, rows, ln_w, ln_b, eps,
                     proj, D, l2norm, out);
    MMVID_LAUNCH_CHECK("clip_pool_project");
    return MMVID_OK;
}

extern "C" int mmvid_clip_pair_scores(const float* img, const float* txt, int B, int T, int D, float* out, void* stream) {
    MMVID_REQUIRE(img && txt && out, "clip_pair_scores: null pointer");
    MMVID_REQUIRE(B > 0 && T > 0 && D > 0, "clip_pair_scores: bad sizes B=%d T=%d D=%d", B, T, D);
    const int64_t BT = (int64_t)B * T;
    hipLaunchKernelGGL(clip_pair_scores_kernel, dim3((unsigned)((BT + 3) / 4)), dim3(256), 0, (hipStream_t)stream, img, txt, BT, T, D, out);
    MMVID_LAUNCH_CHECK("clip_pair_scores");
    return MMVID_OK;
}
