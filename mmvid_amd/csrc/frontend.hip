// Stochastic front-end of a BERT training step as device code (SURVEY next-row N2): the reference draws these on the
// host, per sample, from four different RNGs (numpy, `random`, torch, torchvision) inside forward():
//   MSM masking strategies        mmvid_pytorch/dalle_bert.py:992-1029  (Bernoulli / full / RandomErasing box / inverse box,
//                                 optional frame preservation 1022-1026)
//   VID negative `warp()`         dalle_bert.py:204-238  (frame from another sample / frame shuffle / colour shift /
//                                 affine warp of one frame, 93-202)
//   visual-token erasing          dalle_bert.py:779-848  (random_erase_codebook, erase_codebook_face)
// Here one counter-based generator (Philox4x32-10) keyed by (seed, step, sample, purpose) makes every decision on the
// device: the captured training step replays without host input, and two ranks with different seeds draw different
// streams.  The reference's streams cannot be reproduced bit for bit (torchvision is unpinned, numpy/python generators
// do not exist on the device); what is restated is each DISTRIBUTION, checked statistically in tests/ against
// oracle/frontend.py.  All kernels are elementwise / tiny: HBM-bound.
#include "../../include/mmvid_hip.h"
#include "common.h"
#include "philox.h"
#include "step_state.h"

namespace {

// ---- Philox4x32-10 and the word-to-uniform mapping u01: philox.h -------------------------------------------------
struct Rng {  // one stream = (seed, step, sample, purpose); draw i of the stream = word (i & 3) of block (i >> 2)
    uint32_t k0, k1, step, sample, purpose;
    __device__ __forceinline__ float uniform(uint32_t i) const {
        const U4 r = philox(i >> 2, purpose, sample, step, k0, k1);
        const uint32_t w = (i & 3) == 0 ? r.x : ((i & 3) == 1 ? r.y : ((i & 3) == 2 ? r.z : r.w));
        return u01(w);
    }
};
__device__ __forceinline__ Rng make_rng(uint64_t seed, const float* step_dev, int sample, int purpose) {
    Rng g;
    g.k0 = (uint32_t)seed, g.k1 = (uint32_t)(seed >> 32);
    g.step = 0u;
    if (step_dev) {  // front-end state: {forward-call counter (fp32), seed low word, seed high word, reserved}
        g.step = (uint32_t)step_dev[0];
        g.k0 ^= __float_as_uint(step_dev[1]), g.k1 ^= __float_as_uint(step_dev[2]);
    }
    g.sample = (uint32_t)sample, g.purpose = (uint32_t)purpose;
    return g;
}
enum { P_STRATEGY = 1, P_BERNOULLI = 2, P_BOX = 3, P_PC = 4, P_WARP = 5, P_PERM = 6, P_ERASE = 7, P_FACE = 8, P_VCOLOR = 9,
       P_NULL_TEXT = 10, P_NULL_VISUAL = 11 };

// torchvision.transforms.RandomErasing.get_params (third-party, absent from /root/reference; restated from the
// published semantics): up to 10 attempts of { area*U(scale), exp(U(log ratio)) -> h, w = round(sqrt(..)) ; accept if
// h < H and w < W ; top-left uniform over the valid offsets }.  Returns false when no attempt fits (nothing erased).
__device__ bool erasing_box(const Rng& g, uint32_t base, int H, int W, float s0, float s1, float r0, float r1, int& bi, int& bj,
                            int& bh, int& bw) {
    const float area = (float)(H * W), l0 = logf(r0), l1 = logf(r1);
    for (int a = 0; a < 10; ++a) {
        const float ea = area * (s0 + (s1 - s0) * g.uniform(base + 4 * a));
        const float ar = expf(l0 + (l1 - l0) * g.uniform(base + 4 * a + 1));
        const int h = (int)rintf(sqrtf(ea * ar)), w = (int)rintf(sqrtf(ea / ar));
        if (!(h < H && w < W)) continue;
        bi = (int)(g.uniform(base + 4 * a + 2) * (float)(H - h + 1));
        bj = (int)(g.uniform(base + 4 * a + 3) * (float)(W - w + 1));
        if (bi > H - h) bi = H - h;
        if (bj > W - w) bj = W - w;
        bh = h, bw = w;
        return true;
    }
    return false;
}

// ---- MSM masks: one block per sample.  mask1[b, t*f*f + y*f + x] = 1 where the target token stays VISIBLE.
__global__ __launch_bounds__(256) void msm_mask_kernel(uint64_t seed, const float* __restrict__ step_dev, int T, int f,
                                                       float p1, float p2, float p3, float bern_lo, float bern_hi,
                                                       float pc_prob, unsigned char* __restrict__ mask1,
                                                       float* __restrict__ nfm, int* __restrict__ strategy_out,
                                                       const int* __restrict__ inject,
                                                       const unsigned char* __restrict__ bern_inject) {
    __shared__ int s_strat, s_box[4], s_hasbox;
    __shared__ float s_p;
    __shared__ unsigned char s_keep_frame[64];
    const int b = blockIdx.x, TS = T * f * f;
    if (threadIdx.x == 0 && inject) {  // tests: the decisions of a reference run instead of draws (MSM_INJECT_WORDS per sample:
        const int* d = inject + (long)b * 72;  // strategy, has_box, box i, j, h, w, 2 reserved, keep_frame[64])
        s_strat = d[0], s_hasbox = d[1], s_p = 0.f;
        s_box[0] = d[2], s_box[1] = d[3], s_box[2] = d[4], s_box[3] = d[5];
        for (int t = 0; t < 64; ++t) s_keep_frame[t] = (t < T && d[8 + t]) ? 1 : 0;
        nfm[b] = d[0] == 2 ? 0.f : 1.f;
        if (strategy_out) strategy_out[b] = d[0];
    } else if (threadIdx.x == 0) {
        const Rng g = make_rng(seed, step_dev, b, P_STRATEGY);
        const float u = g.uniform(0);
        const int strat = u < p1 ? 1 : (u < p1 + p2 ? 2 : (u < p1 + p2 + p3 ? 3 : 4));  // np.random.choice([1,2,3,4], p)
        s_strat = strat;
        s_p = bern_lo + (bern_hi - bern_lo) * g.uniform(1);  // np.random.uniform(*msm_bernoulli_prob)
        s_hasbox = 0;
        if (strat >= 3) {
            int bi = 0, bj = 0, bh = 0, bw = 0;
            const Rng gb = make_rng(seed, step_dev, b, P_BOX);
            s_hasbox = erasing_box(gb, 0, f, f, 0.2f, 0.8f, 0.5f, 2.0f, bi, bj, bh, bw) ? 1 : 0;  // dalle_bert.py:290-294
            s_box[0] = bi, s_box[1] = bj, s_box[2] = bh, s_box[3] = bw;
        }
        nfm[b] = strat == 2 ? 0.f : 1.f;
        if (strategy_out) strategy_out[b] = strat;
        for (int t = 0; t < T && t < 64; ++t) s_keep_frame[t] = 0;
        if (pc_prob > 0.f) {  // 1022-1026: with probability pc_prob keep randint(1, T//2) whole frames visible
            const Rng gp = make_rng(seed, step_dev, b, P_PC);
            if (gp.uniform(0) < pc_prob && T >= 2) {
                int cnt = 1 + (int)(gp.uniform(1) * (float)(T / 2));
                if (cnt > T / 2) cnt = T / 2;
                for (int t = 0; t < T && t < 64; ++t) {  // the cnt frames with the smallest draws = a uniform cnt-subset
                    const float ut = gp.uniform(2 + t);
                    int rank = 0;
                    for (int q = 0; q < T; ++q) {
                        const float uq = gp.uniform(2 + q);
                        rank += (uq < ut || (uq == ut && q < t)) ? 1 : 0;
                    }
                    s_keep_frame[t] = rank < cnt ? 1 : 0;
                }
            }
        }
    }
    __syncthreads();
    const int strat = s_strat;
    const Rng gbern = make_rng(seed, step_dev, b, P_BERNOULLI);
    for (int p = threadIdx.x; p < TS; p += 256) {
        const int t = p / (f * f), rem = p - t * f * f, y = rem / f, x = rem - y * f;
        unsigned char m;
        if (strat == 1) {
            m = bern_inject ? bern_inject[(long)b * TS + p] : (gbern.uniform(p) < s_p ? 1 : 0);  // torch.bernoulli(ones * p)
        } else if (strat == 2) {
            m = 0;
        } else {
            const bool inside = s_hasbox && y >= s_box[0] && y < s_box[0] + s_box[2] && x >= s_box[1] && x < s_box[1] + s_box[3];
            m = strat == 3 ? (inside ? 0 : 1) : (inside ? 1 : 0);  // erased box hidden / only the box visible
        }
        if (t < 64 && s_keep_frame[t]) m = 1;
        mask1[(long)b * TS + p] = m;
    }
}

// ---- VID negative: per-sample parameters, then one elementwise pass over the frames
struct WarpParams {  // one per sample
    int mode, j1, src_b, src_t, chan;
    float shift, th[6];
    int perm[32];
};

__global__ void warp_params_kernel(uint64_t seed, const float* __restrict__ step_dev, int B, int T, float p0, float p1, float p2,
                                   WarpParams* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Rng g = make_rng(seed, step_dev, b, P_WARP);
    WarpParams w;
    const float u = g.uniform(0);
    w.mode = u < p0 ? 0 : (u < p0 + p1 ? 1 : (u < p0 + p1 + p2 ? 2 : 3));  // np.random.choice(range(4), p=vid_strategy_prob)
    w.j1 = (int)(g.uniform(1) * (float)T);
    if (w.j1 >= T) w.j1 = T - 1;
    w.src_b = b, w.src_t = w.j1, w.chan = 0, w.shift = 0.f;
    for (int t = 0; t < 32; ++t) w.perm[t] = t;
    for (int e = 0; e < 6; ++e) w.th[e] = 0.f;
    if (w.mode == 0) {  // a frame of another sample (210-217); a batch of one has no "other": keep the frame
        if (B > 1) {
            int o = (int)(g.uniform(2) * (float)(B - 1));
            if (o >= B - 1) o = B - 2;
            w.src_b = o >= b ? o + 1 : o;
        }
        w.src_t = (int)(g.uniform(3) * (float)T);
        if (w.src_t >= T) w.src_t = T - 1;
    } else if (w.mode == 1) {  // a non-identity permutation of the frames (93-108, 218-219)
        const Rng gp = make_rng(seed, step_dev, b, P_PERM);
        for (int attempt = 0; attempt < 16; ++attempt) {
            for (int t = 0; t < T; ++t) w.perm[t] = t;
            for (int t = T - 1; t > 0; --t) {  // Fisher-Yates
                int r = (int)(gp.uniform(attempt * 32 + t) * (float)(t + 1));
                if (r > t) r = t;
                const int tmp = w.perm[t];
                w.perm[t] = w.perm[r], w.perm[r] = tmp;
            }
            bool ident = true;
            for (int t = 0; t < T; ++t) ident = ident && w.perm[t] == t;
            if (!ident || T < 2) break;
        }
    } else if (w.mode == 2) {  // colour shift of one frame (124-135): all channels or one of them
        w.shift = g.uniform(2) - 0.5f;
        w.chan = (int)(g.uniform(3) * 4.0f);
        if (w.chan > 3) w.chan = 3;
    } else {  // affine warp of one frame (168-202 with angle 30, trans 0.1, scale 0.1)
        const float ang = 3.14159265358979323846f * 30.0f / 180.0f;
        const float a = -ang + 2.f * ang * g.uniform(2);
        const float t1 = -0.1f + 0.2f * g.uniform(3), t2 = -0.1f + 0.2f * g.uniform(4);
        const float sc = 0.9f + 0.2f * g.uniform(5);
        w.th[0] = sc * cosf(a), w.th[1] = sc * sinf(-a), w.th[2] = t1;
        w.th[3] = sc * sinf(a), w.th[4] = sc * cosf(a), w.th[5] = t2;
    }
    out[b] = w;
}

__device__ __forceinline__ float reflect_coord(float in, float twice_low, float twice_high) {  // ATen GridSampler.h
    if (twice_low == twice_high) return 0.f;
    const float mn = twice_low * 0.5f, span = (twice_high - twice_low) * 0.5f;
    in = fabsf(in - mn);
    const float extra = fmodf(in, span);
    const int flips = (int)floorf(in / span);
    return (flips & 1) ? span - extra + mn : extra + mn;
}

// F.affine_grid(theta, size, align_corners=False) + F.grid_sample(bilinear, padding_mode='reflection', align_corners=False)
// `px(i)` = pixel i of the source plane: an fp32 load, or a uint8 load converted at load time (warp_new_frame_u8_kernel) -- one body,
// so both sources go through the same operations in the same order.
template <class Px>
__device__ __forceinline__ float affine_sample_px(Px px, int H, int W, const float* th, int y, int x) {
    const float xn = (2.f * x + 1.f) / (float)W - 1.f, yn = (2.f * y + 1.f) / (float)H - 1.f;
    const float gx = th[0] * xn + th[1] * yn + th[2], gy = th[3] * xn + th[4] * yn + th[5];
    float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    ix = fminf(fmaxf(reflect_coord(ix, -1.f, 2.f * W - 1.f), 0.f), (float)(W - 1));
    iy = fminf(fmaxf(reflect_coord(iy, -1.f, 2.f * H - 1.f), 0.f), (float)(H - 1));
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = ix - x0f, wy1 = iy - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    float v = 0.f;
    if (x0 >= 0 && x0 < W && y0 >= 0 && y0 < H) v += px(y0 * W + x0) * wx0 * wy0;
    if (x1 >= 0 && x1 < W && y0 >= 0 && y0 < H) v += px(y0 * W + x1) * wx1 * wy0;
    if (x0 >= 0 && x0 < W && y1 >= 0 && y1 < H) v += px(y1 * W + x0) * wx0 * wy1;
    if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H) v += px(y1 * W + x1) * wx1 * wy1;
    return v;
}
__device__ __forceinline__ float affine_sample(const float* __restrict__ img, int H, int W, const float* th, int y, int x) {
    return affine_sample_px([img](int i) { return img[i]; }, H, W, th, y, x);
}

// x, out: [B, T, C, H, W] fp32.  One thread per output pixel.
__global__ __launch_bounds__(256) void warp_apply_kernel(const float* __restrict__ x, const WarpParams* __restrict__ wp, int B,
                                                         int T, int C, int H, int W, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long hw = (long)H * W, per_b = (long)T * C * hw;
    if (idx >= (long)B * per_b) return;
    const int b = (int)(idx / per_b);
    long r = idx - (long)b * per_b;
    const int t = (int)(r / (C * hw));
    r -= (long)t * C * hw;
    const int c = (int)(r / hw);
    const int pix = (int)(r - (long)c * hw);
    const WarpParams& w = wp[b];
    float v;
    if (w.mode == 1) {
        v = x[(((long)b * T + w.perm[t]) * C + c) * hw + pix];
    } else if (t != w.j1) {
        v = x[idx];
    } else if (w.mode == 0) {
        v = x[(((long)w.src_b * T + w.src_t) * C + c) * hw + pix];
    } else if (w.mode == 2) {
        const float m = (w.chan == 0 || w.chan - 1 == c) ? w.shift : 0.f;
        v = fminf(fmaxf(x[idx] + m, 0.f), 1.f);
    } else {
        v = affine_sample(x + (((long)b * T + t) * C + c) * hw, H, W, w.th, pix / W, pix % W);
    }
    out[idx] = v;
}

// The VID negative differs from the target in ONE frame per sample (modes 0, 2, 3) or is a permutation of its frames
// (mode 1), and the VQGAN encodes frames independently.  So only the frames that are NEW pixels need encoding: one per
// sample (the colour-shifted / affine-warped frame; for modes 0 and 1 the slot is filled with frame j1 and its tokens
// are not used).  new_frames: [B, C, H, W].
__global__ __launch_bounds__(256) void warp_new_frame_kernel(const float* __restrict__ x, const WarpParams* __restrict__ wp, int B,
                                                             int T, int C, int H, int W, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long hw = (long)H * W;
    if (idx >= (long)B * C * hw) return;
    const int b = (int)(idx / (C * hw));
    const long r = idx - (long)b * C * hw;
    const int c = (int)(r / hw);
    const int pix = (int)(r - (long)c * hw);
    const WarpParams& w = wp[b];
    const float* src = x + (((long)b * T + w.j1) * C + c) * hw;
    float v;
    if (w.mode == 2) {
        const float m = (w.chan == 0 || w.chan - 1 == c) ? w.shift : 0.f;
        v = fminf(fmaxf(src[pix] + m, 0.f), 1.f);
    } else if (w.mode == 3) {
        v = affine_sample(src, H, W, w.th, pix / W, pix % W);
    } else {
        v = src[pix];
    }
    out[idx] = v;
}
// ---- uint8 input side (training from a token cache: mmvid_amd/token_cache.py).  Image decoders deliver [H, W, 3] bytes; the
// data path turns them into floats as torchvision's ToTensor does: float(u8) / 255 -- a correctly rounded DIVISION (a multiply
// by 1/255 differs in the last bit for some of the 256 values).
__device__ __forceinline__ float u8_unit(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

struct U3 {
    uint32_t a, b, c;
};
// in [N, HW, 3] uint8 -> out [N, 3, HW] fp32.  VEC: HW % 4 == 0 and `in` 4-byte aligned -- a thread converts 4 pixels: 12
// contiguous bytes in (a wave reads 768 contiguous bytes), one float4 out per channel plane (a wave writes 1 KiB runs).
template <bool VEC>
__global__ __launch_bounds__(256) void frames_u8_to_f32_kernel(const unsigned char* __restrict__ in, long N, long HW,
                                                               float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const long q = HW >> 2;  // groups of 4 pixels per frame
        if (idx >= N * q) return;
        const long n = idx / q, g = idx - n * q;
        const U3 w = *reinterpret_cast<const U3*>(in + (n * HW + 4 * g) * 3);
        const unsigned by[12] = {w.a & 255u, (w.a >> 8) & 255u, (w.a >> 16) & 255u, w.a >> 24, w.b & 255u, (w.b >> 8) & 255u,
                                 (w.b >> 16) & 255u, w.b >> 24, w.c & 255u, (w.c >> 8) & 255u, (w.c >> 16) & 255u, w.c >> 24};
        float* dst = out + n * 3 * HW + 4 * g;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(dst + c * HW) =
                make_float4(u8_unit(by[c]), u8_unit(by[3 + c]), u8_unit(by[6 + c]), u8_unit(by[9 + c]));
    } else {
        if (idx >= N * HW) return;
        const long n = idx / HW, p = idx - n * HW;
        const unsigned char* src = in + idx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(n * 3 + c) * HW + p] = u8_unit(src[c]);
    }
}

// warp_new_frame_kernel on uint8 frames x [B, T, H, W, 3]: a pixel becomes u8 / 255 when it is loaded, everything after that is
// the fp32 kernel's arithmetic (same colour shift, same affine_sample_px body) -> bit-identical to the fp32 kernel on x / 255.
__global__ __launch_bounds__(256) void warp_new_frame_u8_kernel(const unsigned char* __restrict__ x, const WarpParams* __restrict__ wp,
                                                                int B, int T, int H, int W, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long hw = (long)H * W;
    if (idx >= (long)B * 3 * hw) return;
    const int b = (int)(idx / (3 * hw));
    const long r = idx - (long)b * 3 * hw;
    const int c = (int)(r / hw);
    const int pix = (int)(r - (long)c * hw);
    const WarpParams& w = wp[b];
    const unsigned char* src = x + ((long)b * T + w.j1) * hw * 3 + c;
    float v;
    if (w.mode == 2) {
        const float m = (w.chan == 0 || w.chan - 1 == c) ? w.shift : 0.f;
        v = fminf(fmaxf(u8_unit(src[3 * pix]) + m, 0.f), 1.f);
    } else if (w.mode == 3) {
        v = affine_sample_px([src](int i) { return u8_unit(src[3 * i]); }, H, W, w.th, pix / W, pix % W);
    } else {
        v = u8_unit(src[3 * pix]);
    }
    out[idx] = v;
}

// ---- a dataset's tokens resident in HBM: table [F, n] uint16, frame_index [rows] int64 -> out [rows, n] int64.  A row outside
// [0, F) reads row 0 and is counted (faults[2], mmvid_device_faults).  VEC: n % 4 == 0 and the table 8-byte aligned -- a thread
// moves 4 tokens: one 8-byte load, two 16-byte stores.
template <bool VEC>
__global__ __launch_bounds__(256) void token_rows_gather_kernel(const unsigned short* __restrict__ table, long F,
                                                                const long long* __restrict__ frame_index, long rows, int n,
                                                                long long* __restrict__ out, unsigned long long* __restrict__ faults) {
    const int per = VEC ? (n >> 2) : n;  // threads per row
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * per) return;
    const long row = idx / per;
    const int p = (int)(idx - row * per);
    long long f = frame_index[row];
    if (f < 0 || f >= F) {  // never fault; counted once per bad row
        if (p == 0 && faults) atomicAdd(&faults[2], 1ull);
        f = 0;
    }
    if (VEC) {
        const uint2 w = *reinterpret_cast<const uint2*>(table + f * n + 4 * p);
        longlong2* dst = reinterpret_cast<longlong2*>(out + row * n + 4 * p);
        longlong2 lo, hi;
        lo.x = (long long)(w.x & 0xffffu), lo.y = (long long)(w.x >> 16);
        hi.x = (long long)(w.y & 0xffffu), hi.y = (long long)(w.y >> 16);
        dst[0] = lo, dst[1] = hi;
    } else {
        out[row * n + p] = (long long)table[f * n + p];
    }
}

// tokens of the VID negative from the target's tokens [B, T*n] and the new frames' tokens [B, n]
__global__ __launch_bounds__(256) void warp_tokens_kernel(const long long* __restrict__ tok, const long long* __restrict__ extra,
                                                          const WarpParams* __restrict__ wp, int B, int T, int n,
                                                          long long* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * T * n) return;
    const int b = (int)(idx / ((long)T * n));
    const int r = (int)(idx - (long)b * T * n);
    const int t = r / n, p = r - t * n;
    const WarpParams& w = wp[b];
    long long v;
    if (w.mode == 1)
        v = tok[((long)b * T + w.perm[t]) * n + p];
    else if (t != w.j1)
        v = tok[idx];
    else if (w.mode == 0)
        v = tok[((long)w.src_b * T + w.src_t) * n + p];
    else
        v = extra[(long)b * n + p];
    out[idx] = v;
}

// ---- visual-token erasing on [B, Tv, f, f] int64 token maps
// choice c (drawn once per call, as the reference's single random draw per forward): mode 0 = untouched, 1 = keep only
// the box (everything else -> value), 2 = erase the box.  frame0_full: frame 0 is never touched (face2 / face3 modes).
struct EraseChoice {
    float cum[4];
    int mode[4], box[4][4];  // r0, r1, c0, c1 (half-open)
    int n, frame0_full;
};
__global__ __launch_bounds__(256) void erase_choice_kernel(uint64_t seed, const float* __restrict__ step_dev, EraseChoice ch,
                                                           int B, int Tv, int f, long long value, long long* __restrict__ tok) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)B * Tv * f * f;
    if (idx >= total) return;
    const Rng g = make_rng(seed, step_dev, 0, P_FACE);
    const float u = g.uniform(0);
    int c = ch.n - 1;
    for (int i = 0; i < ch.n; ++i)
        if (u < ch.cum[i]) {
            c = i;
            break;
        }
    if (ch.mode[c] == 0) return;
    const int x = (int)(idx % f), y = (int)((idx / f) % f), t = (int)((idx / ((long)f * f)) % Tv);
    if (ch.frame0_full && t == 0) return;
    const bool inside = y >= ch.box[c][0] && y < ch.box[c][1] && x >= ch.box[c][2] && x < ch.box[c][3];
    if ((ch.mode[c] == 1 && !inside) || (ch.mode[c] == 2 && inside)) tok[idx] = value;
}

// random_erase_codebook (779-794): per sample RandomErasing(p, scale, ratio, value) on the [Tv, f, f] map (the same box
// on every frame); erase_half: rows f/2.. of every frame instead.
__global__ __launch_bounds__(256) void random_erase_tokens_kernel(uint64_t seed, const float* __restrict__ step_dev, int Tv,
                                                                  int f, float p, float s0, float s1, float r0, float r1,
                                                                  int erase_half, long long value, long long* __restrict__ tok) {
    __shared__ int s_box[4], s_on;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        s_on = 0;
        if (erase_half) {
            s_box[0] = f / 2, s_box[1] = 0, s_box[2] = f - f / 2, s_box[3] = f, s_on = 1;
        } else {
            const Rng g = make_rng(seed, step_dev, b, P_ERASE);
            if (g.uniform(0) < p) {  // torchvision: `if torch.rand(1) < self.p`
                int bi = 0, bj = 0, bh = 0, bw = 0;
                if (erasing_box(g, 4, f, f, s0, s1, r0, r1, bi, bj, bh, bw)) s_box[0] = bi, s_box[1] = bj, s_box[2] = bh, s_box[3] = bw, s_on = 1;
            }
        }
    }
    __syncthreads();
    if (!s_on) return;
    const int n = Tv * f * f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int x = i % f, y = (i / f) % f;
        if (y >= s_box[0] && y < s_box[0] + s_box[2] && x >= s_box[1] && x < s_box[1] + s_box[3]) tok[(long)b * n + i] = value;
    }
}

// visual_aug_mode == 'motion_color' (dalle_bert.py:140-158, 940-943; dalle_artv.py:460-463): with probability p -- ONE draw
// per forward call, `random.random() < 0.9` -- every sample's visual frames first_frame.. get the same per-sample colour
// shift c ~ U(-0.5, 0.5) on all channels or on one of them (random.randint(0, 3)), clamped to [0, 1]; earlier frames and a
// failed gate leave the pixels untouched.  x [B, Tv, C, H, W] fp32, in place.  params_out (optional, tests): per sample
// {gate, shift, chan}.
__global__ __launch_bounds__(256) void visual_color_kernel(uint64_t seed, const float* __restrict__ step_dev, int B, int Tv, int C,
                                                           long hw, float p, int first_frame, float* __restrict__ x,
                                                           float* __restrict__ params_out) {
    const long per_b = (long)Tv * C * hw;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * per_b) return;
    const int b = (int)(idx / per_b);
    const long r = idx - (long)b * per_b;
    const int t = (int)(r / (C * hw)), c = (int)((r - (long)t * C * hw) / hw);
    const Rng gate = make_rng(seed, step_dev, 0, P_VCOLOR);
    const bool on = gate.uniform(0) < p;
    const Rng g = make_rng(seed, step_dev, b + 1, P_VCOLOR);
    const float shift = g.uniform(0) - 0.5f;
    int chan = (int)(g.uniform(1) * 4.0f);
    if (chan > 3) chan = 3;
    if (params_out && r == 0) params_out[3 * b] = on ? 1.f : 0.f, params_out[3 * b + 1] = shift, params_out[3 * b + 2] = (float)chan;
    if (!on || t < first_frame) return;
    const float m = (chan == 0 || chan - 1 == c) ? shift : 0.f;
    x[idx] = fminf(fmaxf(x[idx] + m, 0.f), 1.f);
}

// ---- condition drop for classifier-free guidance: one block per sample.  With probability p_text the sample's text becomes all pad
// (0: bert_build_ids maps it to the per-position pad ids, dalle_bert.py:917-919), with probability p_visual its visual tokens become
// all [MASK], [SEP] slots included -- what visual=None gives (dalle_bert.py:954-958; train.py:302 --dropout_vc).  Two streams of their
// own: no other decision of the step moves.  `inject` [B, 2] replaces the draws (tests).  Out of place: the inputs may be the caller's.
__global__ __launch_bounds__(256) void cond_drop_kernel(uint64_t seed, const float* __restrict__ step_dev,
                                                        const long long* __restrict__ text, const long long* __restrict__ vis_tok, int Tt,
                                                        int Vs, float p_text, float p_visual, const unsigned char* __restrict__ inject,
                                                        long long mask_id, long long* __restrict__ text_out,
                                                        long long* __restrict__ vis_out, unsigned char* __restrict__ decided) {
    __shared__ int s_drop[2];
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int dt, dv;
        if (inject) {
            dt = inject[2 * b] ? 1 : 0, dv = inject[2 * b + 1] ? 1 : 0;
        } else {
            dt = make_rng(seed, step_dev, b, P_NULL_TEXT).uniform(0) < p_text ? 1 : 0;
            dv = make_rng(seed, step_dev, b, P_NULL_VISUAL).uniform(0) < p_visual ? 1 : 0;
        }
        s_drop[0] = dt, s_drop[1] = dv;
        decided[2 * b] = (unsigned char)dt, decided[2 * b + 1] = (unsigned char)dv;
    }
    __syncthreads();
    const bool dt = s_drop[0] != 0, dv = s_drop[1] != 0;
    for (int i = threadIdx.x; i < Tt; i += 256) text_out[(long)b * Tt + i] = dt ? 0 : text[(long)b * Tt + i];
    if (vis_tok)
        for (int i = threadIdx.x; i < Vs; i += 256) vis_out[(long)b * Vs + i] = dv ? mask_id : vis_tok[(long)b * Vs + i];
}

__global__ void counter_add_kernel(float* c, float v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) c[0] += v;
}

// Learning-rate schedule as a device scalar (utils_train.py:373-385 -> deepspeed WarmupLR, third-party: restated from
// its published semantics).  *step_dev counts finished optimiser steps; the reference calls scheduler.step() after
// every `every`-th iteration (train.py:373-374), so at iteration i the scheduler has been stepped ns = i / every times:
// ns == 0 -> the optimiser's construction lr; else lr = min + (max - min) * gamma(ns - 1),
// gamma(k) = k < warmup ? log(k + 1) / log(warmup) : 1.   kind 0 = constant lr_max.
__global__ void lr_schedule_kernel(const float* __restrict__ step_dev, int kind, float lr_min, float lr_max, int warmup,
                                   int every, float* __restrict__ lr_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float lr = lr_max;
    if (kind == 1) {
        const long it = (long)step_dev[0];
        const long ns = it / (every > 0 ? every : 1);
        if (ns > 0) {
            const long k = ns - 1;
            const long wu = warmup_clamped(warmup);
            const float gamma = k < wu ? warmup_log_gamma(k, wu) : 1.0f;  // (step_state.h: shared with mmvid_lr_schedule_ext)
            lr = lr_min + (lr_max - lr_min) * gamma;
        }
    }
    lr_out[0] = lr;
}

}  // namespace

extern "C" int mmvid_msm_masks(uint64_t seed, const float* step_dev, int B, int T, int f, const float* strategy_prob,
                               float bern_lo, float bern_hi, float pc_prob, uint8_t* mask1, float* not_fully_masked,
                               int32_t* strategy_out, void* stream) {
    MMVID_REQUIRE(strategy_prob && mask1 && not_fully_masked && B > 0 && T > 0 && T <= 64 && f > 0, "msm_masks: bad arguments");
    hipLaunchKernelGGL(msm_mask_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, seed, step_dev, T, f, strategy_prob[0],
                       strategy_prob[1], strategy_prob[2], bern_lo, bern_hi, pc_prob, mask1, not_fully_masked, strategy_out,
                       (const int*)nullptr, (const unsigned char*)nullptr);
    MMVID_LAUNCH_CHECK("msm_masks");
    return MMVID_OK;
}

extern "C" int mmvid_msm_masks_inject(const int32_t* decisions, const uint8_t* bernoulli, int B, int T, int f, uint8_t* mask1,
                                      float* not_fully_masked, void* stream) {
    MMVID_REQUIRE(decisions && mask1 && not_fully_masked && B > 0 && T > 0 && T <= 64 && f > 0, "msm_masks_inject: bad arguments");
    hipLaunchKernelGGL(msm_mask_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (uint64_t)0, (const float*)nullptr, T, f, 0.f, 0.f,
                       0.f, 0.f, 0.f, 0.f, mask1, not_fully_masked, (int*)nullptr, decisions, bernoulli);
    MMVID_LAUNCH_CHECK("msm_masks_inject");
    return MMVID_OK;
}

extern "C" int mmvid_warp_params_bytes(void) { return (int)sizeof(WarpParams); }

extern "C" int mmvid_vid_warp(uint64_t seed, const float* step_dev, const float* x, int B, int T, int C, int H, int W,
                              const float* strategy_prob, void* params_scratch, int draw_params, float* out, void* stream) {
    MMVID_REQUIRE(x && strategy_prob && params_scratch && out, "vid_warp: null pointer");
    MMVID_REQUIRE(B > 0 && T > 0 && T <= 32, "vid_warp: B=%d T=%d (T <= 32)", B, T);
    hipStream_t s = (hipStream_t)stream;
    if (draw_params)
        hipLaunchKernelGGL(warp_params_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, seed, step_dev, B, T, strategy_prob[0],
                           strategy_prob[1], strategy_prob[2], (WarpParams*)params_scratch);
    const long total = (long)B * T * C * H * W;
    hipLaunchKernelGGL(warp_apply_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, x, (const WarpParams*)params_scratch, B, T, C, H,
                       W, out);
    MMVID_LAUNCH_CHECK("vid_warp");
    return MMVID_OK;
}

extern "C" int mmvid_vid_warp_new_frames(uint64_t seed, const float* step_dev, const float* x, int B, int T, int C, int H, int W,
                                         const float* strategy_prob, void* params_scratch, int draw_params, float* new_frames,
                                         void* stream) {
    MMVID_REQUIRE(x && strategy_prob && params_scratch && new_frames, "vid_warp_new_frames: null pointer");
    MMVID_REQUIRE(B > 0 && T > 0 && T <= 32, "vid_warp_new_frames: B=%d T=%d (T <= 32)", B, T);
    hipStream_t s = (hipStream_t)stream;
    if (draw_params)
        hipLaunchKernelGGL(warp_params_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, seed, step_dev, B, T, strategy_prob[0],
                           strategy_prob[1], strategy_prob[2], (WarpParams*)params_scratch);
    const long total = (long)B * C * H * W;
    hipLaunchKernelGGL(warp_new_frame_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, x, (const WarpParams*)params_scratch, B, T, C,
                       H, W, new_frames);
    MMVID_LAUNCH_CHECK("vid_warp_new_frames");
    return MMVID_OK;
}

extern "C" int mmvid_vid_warp_tokens(const int64_t* target_tok, const int64_t* new_frame_tok, const void* params, int B, int T,
                                     int n, int64_t* out, void* stream) {
    MMVID_REQUIRE(target_tok && new_frame_tok && params && out && B > 0 && T > 0 && n > 0, "vid_warp_tokens: bad arguments");
    const long total = (long)B * T * n;
    hipLaunchKernelGGL(warp_tokens_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)target_tok,
                       (const long long*)new_frame_tok, (const WarpParams*)params, B, T, n, (long long*)out);
    MMVID_LAUNCH_CHECK("vid_warp_tokens");
    return MMVID_OK;
}

extern "C" int mmvid_frames_u8_to_f32(const uint8_t* frames_u8, int N, int H, int W, float* out, void* stream) {
    MMVID_REQUIRE(frames_u8 && out && N >= 0 && H > 0 && W > 0, "frames_u8_to_f32: bad arguments");
    if (N == 0) return MMVID_OK;
    const long hw = (long)H * W;
    if (hw % 4 == 0 && ((uintptr_t)frames_u8 & 3) == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(frames_u8_to_f32_kernel<true>, dim3(cdiv((long)N * (hw / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                           frames_u8, (long)N, hw, out);
    else
        hipLaunchKernelGGL(frames_u8_to_f32_kernel<false>, dim3(cdiv((long)N * hw, 256)), dim3(256), 0, (hipStream_t)stream,
                           frames_u8, (long)N, hw, out);
    MMVID_LAUNCH_CHECK("frames_u8_to_f32");
    return MMVID_OK;
}

extern "C" int mmvid_vid_warp_new_frames_u8(uint64_t seed, const float* step_dev, const uint8_t* x_u8, int B, int T, int H, int W,
                                            const float* strategy_prob, void* params_scratch, int draw_params, float* new_frames,
                                            void* stream) {
    MMVID_REQUIRE(x_u8 && strategy_prob && params_scratch && new_frames, "vid_warp_new_frames_u8: null pointer");
    MMVID_REQUIRE(B > 0 && T > 0 && T <= 32 && H > 0 && W > 0, "vid_warp_new_frames_u8: B=%d T=%d (T <= 32)", B, T);
    hipStream_t s = (hipStream_t)stream;
    if (draw_params)
        hipLaunchKernelGGL(warp_params_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, seed, step_dev, B, T, strategy_prob[0],
                           strategy_prob[1], strategy_prob[2], (WarpParams*)params_scratch);
    const long total = (long)B * 3 * H * W;
    hipLaunchKernelGGL(warp_new_frame_u8_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, x_u8, (const WarpParams*)params_scratch, B, T,
                       H, W, new_frames);
    MMVID_LAUNCH_CHECK("vid_warp_new_frames_u8");
    return MMVID_OK;
}

extern "C" int mmvid_vid_warp_draw(uint64_t seed, const float* step_dev, int B, int T, const float* strategy_prob,
                                   void* params_scratch, void* stream) {
    MMVID_REQUIRE(strategy_prob && params_scratch && B > 0 && T > 0 && T <= 32, "vid_warp_draw: bad arguments");
    hipLaunchKernelGGL(warp_params_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, seed, step_dev, B, T, strategy_prob[0],
                       strategy_prob[1], strategy_prob[2], (WarpParams*)params_scratch);
    MMVID_LAUNCH_CHECK("vid_warp_draw");
    return MMVID_OK;
}

extern "C" int mmvid_token_rows_gather(const uint16_t* table, int64_t table_rows, const int64_t* frame_index, int64_t rows, int n,
                                       int64_t* out, void* stream) {
    MMVID_REQUIRE(table && frame_index && out && table_rows > 0 && rows >= 0 && n > 0, "token_rows_gather: bad arguments");
    if (rows == 0) return MMVID_OK;
    unsigned long long* faults = mmvid_fault_counters_dev();
    MMVID_REQUIRE(faults, "token_rows_gather: the device fault counters are not reachable");
    if (n % 4 == 0 && ((uintptr_t)table & 7) == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(token_rows_gather_kernel<true>, dim3(cdiv((long)rows * (n / 4), 256)), dim3(256), 0, (hipStream_t)stream,
                           table, (long)table_rows, (const long long*)frame_index, (long)rows, n, (long long*)out, faults);
    else
        hipLaunchKernelGGL(token_rows_gather_kernel<false>, dim3(cdiv((long)rows * n, 256)), dim3(256), 0, (hipStream_t)stream, table,
                           (long)table_rows, (const long long*)frame_index, (long)rows, n, (long long*)out, faults);
    MMVID_LAUNCH_CHECK("token_rows_gather");
    return MMVID_OK;
}

extern "C" int mmvid_erase_tokens_choice(uint64_t seed, const float* step_dev, int nchoice, const float* cumprob,
                                         const int32_t* modes, const int32_t* boxes, int frame0_full, int B, int Tv, int f,
                                         int64_t value, int64_t* tok, void* stream) {
    MMVID_REQUIRE(cumprob && modes && boxes && tok && nchoice >= 1 && nchoice <= 4, "erase_tokens_choice: bad arguments");
    EraseChoice ch = {};
    ch.n = nchoice, ch.frame0_full = frame0_full;
    for (int i = 0; i < nchoice; ++i) {
        ch.cum[i] = cumprob[i], ch.mode[i] = modes[i];
        for (int e = 0; e < 4; ++e) ch.box[i][e] = boxes[i * 4 + e];
    }
    const long total = (long)B * Tv * f * f;
    if (total == 0) return MMVID_OK;
    hipLaunchKernelGGL(erase_choice_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, seed, step_dev, ch, B, Tv, f,
                       (long long)value, (long long*)tok);
    MMVID_LAUNCH_CHECK("erase_tokens_choice");
    return MMVID_OK;
}

extern "C" int mmvid_random_erase_tokens(uint64_t seed, const float* step_dev, int B, int Tv, int f, float p, float scale_lo,
                                         float scale_hi, float ratio_lo, float ratio_hi, int erase_half, int64_t value,
                                         int64_t* tok, void* stream) {
    MMVID_REQUIRE(tok && B > 0 && Tv > 0 && f > 0, "random_erase_tokens: bad arguments");
    hipLaunchKernelGGL(random_erase_tokens_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, seed, step_dev, Tv, f, p, scale_lo,
                       scale_hi, ratio_lo, ratio_hi, erase_half, (long long)value, (long long*)tok);
    MMVID_LAUNCH_CHECK("random_erase_tokens");
    return MMVID_OK;
}

extern "C" int mmvid_visual_color_jitter(uint64_t seed, const float* step_dev, float* x, int B, int Tv, int C, int H, int W, float p,
                                         int first_frame, float* params_out, void* stream) {
    MMVID_REQUIRE(x && B > 0 && Tv > 0 && C > 0 && H > 0 && W > 0, "visual_color_jitter: bad arguments");
    const long total = (long)B * Tv * C * H * W;
    hipLaunchKernelGGL(visual_color_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, seed, step_dev, B, Tv, C,
                       (long)H * W, p, first_frame, x, params_out);
    MMVID_LAUNCH_CHECK("visual_color_jitter");
    return MMVID_OK;
}

extern "C" int mmvid_cond_drop(const int64_t* text, const int64_t* vis_tok, int B, int Tt, int Vs, const float* state_dev, uint64_t seed,
                               float p_text, float p_visual, const uint8_t* inject, int64_t mask_id, int64_t* text_out, int64_t* vis_out,
                               uint8_t* decided, void* stream) {
    MMVID_REQUIRE(text && text_out && decided && B > 0 && Tt > 0 && Vs >= 0, "cond_drop: bad arguments");
    MMVID_REQUIRE(!vis_tok || (vis_out && Vs > 0), "cond_drop: visual tokens need vis_out and Vs > 0");
    MMVID_REQUIRE(p_text >= 0.f && p_text <= 1.f && p_visual >= 0.f && p_visual <= 1.f, "cond_drop: p_text=%g p_visual=%g outside [0, 1]",
                  (double)p_text, (double)p_visual);
    hipLaunchKernelGGL(cond_drop_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, seed, state_dev, (const long long*)text,
                       (const long long*)vis_tok, Tt, Vs, p_text, p_visual, inject, (long long)mask_id, (long long*)text_out,
                       (long long*)vis_out, decided);
    MMVID_LAUNCH_CHECK("cond_drop");
    return MMVID_OK;
}

extern "C" int mmvid_counter_add(float* counter, float value, void* stream) {
    MMVID_REQUIRE(counter, "counter_add: null pointer");
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, value);
    MMVID_LAUNCH_CHECK("counter_add");
    return MMVID_OK;
}

extern "C" int mmvid_lr_schedule(const float* step_dev, int kind, float lr_min, float lr_max, int warmup_steps, int every,
                                 float* lr_out, void* stream) {
    MMVID_REQUIRE(step_dev && lr_out, "lr_schedule: null pointer");
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, kind, lr_min, lr_max, warmup_steps,
                       every, lr_out);
    MMVID_LAUNCH_CHECK("lr_schedule");
    return MMVID_OK;
}
