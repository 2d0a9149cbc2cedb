// I3D (InceptionI3d, RGB stream, Kinetics-400) for the FVD / PRD evaluation of utils/utils_eval.py:32-219, for gfx950.
// The reference runs DeepMind's TF-Hub graph through tensorflow.compat.v1 (frechet_video_distance.py:34-83); here:
//   i3d_preprocess_kernel   extend_video + cut (a computed frame map) -> x255 -> TF1 legacy bilinear resize to 224^2 -> 2v/255-1,
//                           written as the stem's folded bf16 operand (below);
//   conv3d_igemm_kernel     every Unit3D (conv3d + folded BatchNorm + ReLU) as implicit GEMM on NDHWC bf16:
//                           M = N*To*Ho*Wo, N_gemm = Cout, K = kt*kh*kw*Cin, k = ((it*kh + ih)*kw + iw)*Cin + ci;
//   maxpool3d_kernel        TF-SAME max pooling, 8 channels (16 B) per thread;
//   i3d_head_kernel         avgpool (2,7,7) VALID + the 1024 -> 400 logits + mean over time, fp32.
// The stem (Cin = 3, 7x7x7, stride 2) would waste 5/8 of every 16-byte channel chunk; the preprocess kernel instead folds (kw, c) into
// the channel axis at the even input columns: folded[n][t][y][wo][3 kw + c] = v[n][t][y][2 wo - pw0 + kw][c] (0 outside, 21..23 = 0),
// so the stem is a 7x7x1 convolution with stride (2, 2, 1) over Cin = 24: K = 1,176 executed against the algorithmic 1,029 (1.14x).
// Same tile machinery as conv.hip (gemm_core.h: 128x128x64 tile, swizzled LDS, LDS-DMA through a range-checked buffer descriptor,
// 32x32x16 bf16 MFMA, fp32 accumulate).  One block shape for every layer and no split-K: a clip's result does not depend on the
// batch it is in.
#include "../../include/mmvid_hip.h"
#include "gemm_core.h"
#include "prof.h"

namespace {
using namespace mmvid_core;

struct Conv3dParams {
    const bf16_t* x;
    const bf16_t* w;
    const float* bias;
    int T, H, W, Cin, To, Ho, Wo, Cout, K;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;  // pt/ph/pw: front pads (the back pads are the range check)
    int M;
    uint32_t xbytes;
    uint32_t mg_cin, mg_kw, mg_kh;  // ceil(2^32 / d) for d > 1: floor(a / d) = umulhi(a, mg) for the a that occur (d = 1: no magic)
    int relu, nseg;
    int seg_end[3], ldo[3], c_off[3];
    bf16_t* out[3];
};

// A-operand gather for a kt x kh x kw window (Cin % 8 == 0: a 16-byte chunk is 8 channels of one tap).  Wave w, piece jj owns tile row
// (4 w + jj) * 8 + (lane >> 3); its LDS slot (lane & 7) holds logical chunk (lane & 7) ^ (4 (jj & 1) + (lane >> 4)) (gemm_core.h's row
// swizzle), so a lane has TWO chunk positions, by the parity of jj.  k -> (tap, ci) -> (it, ih, iw) by multiply-high with magic
// reciprocals (exact here: k * Cin < 2^32), twice per K tile; the stage holds no per-tile state.
__device__ __forceinline__ uint32_t udiv(uint32_t a, uint32_t mg) { return __umulhi(a, mg); }

struct Conv3dAStage {
    int nt[4], t0[4], y0[4], x0[4];  // n*T and the window origin of each piece's output pixel; nt = -1: row beyond M
    int ch[2];                       // this lane's chunk offset (elements) for even / odd pieces
    rsrc_t rsrc;
    __device__ __forceinline__ void init(const Conv3dParams& p, int m0, int wave, int lane) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int m = m0 + (wave * 4 + jj) * 8 + (lane >> 3);
            int r = m < p.M ? m : 0;  // (branch-free: a branch here made the compiler address the arrays dynamically, in scratch)
            const int wo = r % p.Wo;
            r /= p.Wo;
            const int ho = r % p.Ho;
            r /= p.Ho;
            const int to = r % p.To;
            nt[jj] = m < p.M ? (r / p.To) * p.T : -1;
            t0[jj] = to * p.st - p.pt, y0[jj] = ho * p.sh - p.ph, x0[jj] = wo * p.sw - p.pw;
        }
        ch[0] = ((lane & 7) ^ (lane >> 4)) * 8, ch[1] = ((lane & 7) ^ (4 + (lane >> 4))) * 8;
        rsrc = make_rsrc(p.x, p.xbytes);
    }
    __device__ __forceinline__ void issue(const Conv3dParams& p, int k0, char* tile, int wave) const {
        int ci[2], it[2], ih[2], iw[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t k = (uint32_t)(k0 + ch[c]);
            const uint32_t tap = udiv(k, p.mg_cin);
            ci[c] = (int)(k - tap * p.Cin);
            const uint32_t q = p.kw == 1 ? tap : udiv(tap, p.mg_kw);
            iw[c] = (int)(tap - q * p.kw);
            it[c] = (int)(p.kh == 1 ? q : udiv(q, p.mg_kh));
            ih[c] = (int)(q - it[c] * p.kh);
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int c = jj & 1;
            const int t = t0[jj] + it[c], y = y0[jj] + ih[c], x = x0[jj] + iw[c];
            const bool ok = nt[jj] >= 0 && it[c] < p.kt && (unsigned)t < (unsigned)p.T && (unsigned)y < (unsigned)p.H &&
                            (unsigned)x < (unsigned)p.W;
            const uint32_t off = (uint32_t)(((((nt[jj] + t) * p.H + y) * p.W + x) * p.Cin + ci[c]) * 2);
            blds16(rsrc, ok ? off : OOB, 0, tile + (wave * 4 + jj) * 1024);
        }
    }
};

// ONE: a 1x1x1 stride-1 convolution, i.e. a plain GEMM with the activation [M][Cin] as the row-major A operand.
template <bool ONE>
__global__ __launch_bounds__(256, 2) void conv3d_igemm_kernel(Conv3dParams p) {
    using S = BlockShape<2>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int wg = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int bn0 = (wg % gridDim.x) * BN;
    const int bm0 = (wg / gridDim.x) * BM;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    OperandStage<false, 1, S::PPW> sb;  // weights [Cout][K] row-major
    sb.init(p.w, p.K, p.Cout, p.K, bn0, wave, lane);
    const int nt = (p.K + BK - 1) / BK;
    std::conditional_t<ONE, OperandStage<false, 1, S::PPW>, Conv3dAStage> sa;
    if constexpr (ONE)
        sa.init(p.x, p.Cin, p.M, p.Cin, bm0, wave, lane);
    else
        sa.init(p, bm0, wave, lane);
    auto stage_tile = [&](int t, char* buf) {
        if constexpr (ONE)
            sa.issue(t * BK, p.K, buf, wave, lane);
        else
            sa.issue(p, t * BK, buf, wave);
        sb.issue(t * BK, p.K, buf + TILE_BYTES, wave, lane);
    };
    stage_tile(0, smem);
    for (int t = 0; t < nt; ++t) {
        char* cur = smem + (t & 1) * S::STAGE_BYTES;
        char* nxt = smem + ((t + 1) & 1) * S::STAGE_BYTES;
        dma_publish_barrier();
        if (t + 1 < nt) stage_tile(t + 1, nxt);
        mma_tile<false, false>(cur, cur + TILE_BYTES, acc, wm, wn, lane);
    }
    // epilogue through an LDS slab (row-contiguous traffic): a thread finishes 8 channels of a row -> one 16-byte store into the
    // channel slice of the segment that owns those columns (segment ends, ldo and c_off are multiples of 8)
    mfma_settle(acc[0][0]), mfma_settle(acc[0][1]), mfma_settle(acc[1][0]), mfma_settle(acc[1][1]);
    float* slab = reinterpret_cast<float*>(smem);
    const int n = bn0 + 8 * (tid & 15);
    const bool n_ok = n < p.Cout;
    const int seg = n < p.seg_end[0] ? 0 : (n < p.seg_end[1] ? 1 : 2);
    // (selects, not an indexed read of the kernel argument: that would be copied to scratch)
    const int seg0 = seg == 0 ? 0 : (seg == 1 ? p.seg_end[0] : p.seg_end[1]);
    bf16_t* const base = seg == 0 ? p.out[0] : (seg == 1 ? p.out[1] : p.out[2]);
    const int coff = seg == 0 ? p.c_off[0] : (seg == 1 ? p.c_off[1] : p.c_off[2]);
    const long ldo = seg == 0 ? p.ldo[0] : (seg == 1 ? p.ldo[1] : p.ldo[2]);
    bf16_t* dst = base + coff + (n - seg0);
    float bz[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bz[e] = n_ok ? p.bias[n + e] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        __syncthreads();
        slab_write(acc, i, slab, wm, wn, lane);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = (tid + 256 * k) >> 4;
            const int m = bm0 + (r >> 5) * 64 + i * 32 + (r & 31);
            if (!n_ok || m >= p.M) continue;
            const float4 a = *reinterpret_cast<const float4*>(slab + r * SLAB_PITCH + 8 * (tid & 15));
            const float4 b = *reinterpret_cast<const float4*>(slab + r * SLAB_PITCH + 8 * (tid & 15) + 4);
            float v[8] = {a.x + bz[0], a.y + bz[1], a.z + bz[2], a.w + bz[3], b.x + bz[4], b.y + bz[5], b.z + bz[6], b.w + bz[7]};
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            *reinterpret_cast<uint4*>(dst + (long)m * ldo) =
                make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
        }
    }
}

// TF-SAME max pooling: padded taps are ignored (max over the window's in-range taps).  One thread = 8 channels of one output pixel.
__global__ __launch_bounds__(256) void maxpool3d_kernel(const bf16_t* __restrict__ x, int T, int H, int W, int C, int kt, int kh, int kw,
                                                        int st, int sh, int sw, int pt, int ph, int pw, int To, int Ho, int Wo, long total,
                                                        bf16_t* __restrict__ out, int ldo, int c_off) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = C >> 3;
    const int c = (int)(i % c8) * 8;
    long r = i / c8;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    r /= Ho;
    const int to = (int)(r % To);
    const long n = r / To;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    for (int a = 0; a < kt; ++a) {
        const int t = to * st - pt + a;
        if (t < 0 || t >= T) continue;
        for (int b = 0; b < kh; ++b) {
            const int y = ho * sh - ph + b;
            if (y < 0 || y >= H) continue;
            for (int d = 0; d < kw; ++d) {
                const int xx = wo * sw - pw + d;
                if (xx < 0 || xx >= W) continue;
                const uint4 u = *reinterpret_cast<const uint4*>(x + (((n * T + t) * H + y) * W + xx) * C + c);
                const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) m[2 * e] = fmaxf(m[2 * e], bf_lo(uw[e])), m[2 * e + 1] = fmaxf(m[2 * e + 1], bf_hi(uw[e]));
            }
        }
    }
    // the maxima are bf16 values already: the repack is exact
    *reinterpret_cast<uint4*>(out + (((n * To + to) * Ho + ho) * Wo + wo) * (long)ldo + c_off + c) =
        make_uint4(pack_bf2(m[0], m[1]), pack_bf2(m[2], m[3]), pack_bf2(m[4], m[5]), pack_bf2(m[6], m[7]));
}

// the folded stem operand at (n, t, y, wo) from a pixel source px(t, y, x, c) (fp32, preprocessed): 24 bf16 = 3 x 16-byte stores
template <class Px>
__device__ __forceinline__ void store_folded(bf16_t* out, long pos, int wo, int pw0, int Win, Px px) {
    float v[24];
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) {
        const int xx = 2 * wo - pw0 + kw;
        const bool ok = xx >= 0 && xx < Win;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * kw + c] = ok ? px(xx, c) : 0.f;
    }
    v[21] = v[22] = v[23] = 0.f;
    uint4* o = reinterpret_cast<uint4*>(out + pos * 24);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        o[q] = make_uint4(pack_bf2(v[8 * q], v[8 * q + 1]), pack_bf2(v[8 * q + 2], v[8 * q + 3]), pack_bf2(v[8 * q + 4], v[8 * q + 5]),
                          pack_bf2(v[8 * q + 6], v[8 * q + 7]));
}

// utils_eval.py:18-29 + 214-223 and frechet_video_distance.py:34-52.  Thread = one folded position (n, j, y, wo) of [n][VL][224][112].
// Frame j of the extended clip: j < t -> j; past it, segment s = 1 + (j - t) / (t - 1), offset q = (j - t) % (t - 1): odd s is the
// flipped clip without its first frame (t - 2 - q), even s the clip without its first frame (1 + q).
__global__ __launch_bounds__(256) void i3d_preprocess_kernel(const float* __restrict__ v, int t, int h, int w, int VL, long total, int pw0,
                                                             bf16_t* __restrict__ out) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int wo = (int)(i % 112);
    long r = i / 112;
    const int y = (int)(r % 224);
    r /= 224;
    const int j = (int)(r % VL);
    const long n = r / VL;
    int f = j;
    if (j >= t) {
        const int s = 1 + (j - t) / (t - 1), q = (j - t) % (t - 1);
        f = (s & 1) ? t - 2 - q : 1 + q;
    }
    const float* src = v + (n * t + f) * 3l * h * w;
    const float sy = (float)h / 224.f, sx = (float)w / 224.f;  // TF1 legacy: src = dst * in / out
    const float fy = (float)y * sy;
    const int ylo = (int)floorf(fy), yhi = min(ylo + 1, h - 1);
    const float ly = fy - floorf(fy);
    store_folded(out, i, wo, pw0, 224, [&](int xx, int c) {
        const float fx = (float)xx * sx;
        const int xlo = (int)floorf(fx), xhi = min(xlo + 1, w - 1);
        const float lx = fx - floorf(fx);
        const float* pc = src + (long)c * h * w;
        const float tl = pc[(long)ylo * w + xlo] * 255.f, tr = pc[(long)ylo * w + xhi] * 255.f;
        const float bl = pc[(long)yhi * w + xlo] * 255.f, br = pc[(long)yhi * w + xhi] * 255.f;
        const float top = tl + (tr - tl) * lx;
        const float bot = bl + (br - bl) * lx;
        const float val = top + (bot - top) * ly;
        return 2.f * val / 255.f - 1.f;
    });
}

// an already preprocessed [n][T][224][224][3] fp32 clip -> the folded stem operand
__global__ __launch_bounds__(256) void i3d_fold_kernel(const float* __restrict__ v, long total, int pw0, bf16_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int wo = (int)(i % 112);
    const long row = i / 112;  // (n, t, y)
    const float* src = v + row * 224 * 3;
    store_folded(out, i, wo, pw0, 224, [&](int xx, int c) { return src[xx * 3 + c]; });
}

// block = one clip: pooled[tp][c] = mean of the (2, 7, 7) window at time tp (fixed order), then logits[o] = mean over tp of
// (bias[o] + W[o] . pooled[tp]) -- one wave per output, lanes over channels, fp32 throughout
constexpr int HEAD_MAX_TP = 8;
__global__ __launch_bounds__(256) void i3d_head_kernel(const bf16_t* __restrict__ x, int To, int C, const float* __restrict__ w,
                                                       const float* __restrict__ b, int ncls, float* __restrict__ out) {
    extern __shared__ float pooled[];  // [To - 1][C]
    const int n = blockIdx.x, tp_n = To - 1;
    const bf16_t* xc = x + (long)n * To * 49 * C;
    for (int idx = threadIdx.x; idx < tp_n * C; idx += 256) {
        const int tp = idx / C, c = idx - tp * C;
        float s = 0.f;
        for (int dt = 0; dt < 2; ++dt)
            for (int p = 0; p < 49; ++p) s += bf2f(xc[((long)(tp + dt) * 49 + p) * C + c]);
        pooled[idx] = s / 98.f;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int o = wave; o < ncls; o += 4) {
        float acc = 0.f;
        for (int tp = 0; tp < tp_n; ++tp) {
            float d = 0.f;
            for (int c = lane; c < C; c += 64) d += w[(long)o * C + c] * pooled[tp * C + c];
            acc += wave_sum(d) + b[o];
        }
        if (lane == 0) out[(long)n * ncls + o] = acc / (float)tp_n;
    }
}

}  // namespace

extern "C" int mmvid_conv3d_ndhwc(const mmvid_conv3d_t* c, const void* x, const void* w, const float* bias, void* stream) {
    MMVID_REQUIRE(c && x && w && bias, "conv3d_ndhwc: null pointer");
    MMVID_REQUIRE(c->N >= 0 && c->T > 0 && c->H > 0 && c->W > 0 && c->kt > 0 && c->kh > 0 && c->kw > 0 && c->st > 0 && c->sh > 0 &&
                      c->sw > 0,
                  "conv3d_ndhwc: bad geometry");
    MMVID_REQUIRE(c->Cin % 8 == 0 && c->Cin > 0 && c->Cout % 8 == 0 && c->Cout > 0, "conv3d_ndhwc: Cin=%d and Cout=%d must be multiples of 8",
                  c->Cin, c->Cout);
    MMVID_REQUIRE(c->pt0 >= 0 && c->pt1 >= 0 && c->ph0 >= 0 && c->ph1 >= 0 && c->pw0 >= 0 && c->pw1 >= 0 && c->pt0 < c->kt && c->ph0 < c->kh &&
                      c->pw0 < c->kw,
                  "conv3d_ndhwc: bad padding");
    MMVID_REQUIRE(c->nseg >= 1 && c->nseg <= 3 && c->seg_end[c->nseg - 1] == c->Cout, "conv3d_ndhwc: %d segments must end at Cout", c->nseg);
    Conv3dParams p;
    p.To = (c->T + c->pt0 + c->pt1 - c->kt) / c->st + 1;
    p.Ho = (c->H + c->ph0 + c->ph1 - c->kh) / c->sh + 1;
    p.Wo = (c->W + c->pw0 + c->pw1 - c->kw) / c->sw + 1;
    MMVID_REQUIRE(p.To > 0 && p.Ho > 0 && p.Wo > 0, "conv3d_ndhwc: empty output");
    const long M = (long)c->N * p.To * p.Ho * p.Wo, K = (long)c->kt * c->kh * c->kw * c->Cin;
    const long xel = (long)c->N * c->T * c->H * c->W * c->Cin;
    MMVID_REQUIRE(K < (1l << 17), "conv3d_ndhwc: K = %ld taps x channels (the gather's reciprocal division is exact below 2^17)", K);
    MMVID_REQUIRE(xel * 2 < (1l << 31) && (long)c->Cout * K * 2 < (1l << 31), "conv3d_ndhwc: input or weight of 2 GiB or more");
    int prev = 0;
    for (int s = 0; s < c->nseg; ++s) {
        const int width = c->seg_end[s] - prev;
        MMVID_REQUIRE(c->out[s] && width > 0 && width % 8 == 0 && c->ldo[s] % 8 == 0 && c->c_off[s] % 8 == 0 && c->c_off[s] >= 0 &&
                          c->c_off[s] + width <= c->ldo[s],
                      "conv3d_ndhwc: segment %d (columns [%d, %d) -> channels [%d, +%d) of %d) must be 8-aligned and inside its output", s,
                      prev, c->seg_end[s], c->c_off[s], width, c->ldo[s]);
        MMVID_REQUIRE(M * c->ldo[s] * 2 < (1l << 31), "conv3d_ndhwc: output of 2 GiB or more");
        prev = c->seg_end[s];
    }
    p.x = (const bf16_t*)x, p.w = (const bf16_t*)w, p.bias = bias;
    p.T = c->T, p.H = c->H, p.W = c->W, p.Cin = c->Cin, p.Cout = c->Cout, p.K = (int)K, p.M = (int)M;
    p.kt = c->kt, p.kh = c->kh, p.kw = c->kw, p.st = c->st, p.sh = c->sh, p.sw = c->sw, p.pt = c->pt0, p.ph = c->ph0, p.pw = c->pw0;
    p.xbytes = (uint32_t)(xel * 2);
    auto magic = [](uint32_t d) { return (uint32_t)(((1ull << 32) + d - 1) / d); };
    p.mg_cin = magic(c->Cin), p.mg_kw = c->kw > 1 ? magic(c->kw) : 0, p.mg_kh = c->kh > 1 ? magic(c->kh) : 0;
    p.relu = c->relu, p.nseg = c->nseg;
    for (int s = 0; s < 3; ++s) {
        const int q = s < c->nseg ? s : c->nseg - 1;
        p.seg_end[s] = c->seg_end[q], p.ldo[s] = c->ldo[q], p.c_off[s] = c->c_off[q], p.out[s] = (bf16_t*)c->out[q];
    }
    if (M == 0) return MMVID_OK;
    const bool one = c->kt == 1 && c->kh == 1 && c->kw == 1 && c->st == 1 && c->sh == 1 && c->sw == 1;  // (pads < k: all zero)
    MmvidProfScope prof(PROF_CONV, 2.0 * (double)M * c->Cout * K, (hipStream_t)stream);
    using S = BlockShape<2>;
    const dim3 grid(cdiv(c->Cout, BN), cdiv(M, BM));
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)conv3d_igemm_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS_BYTES);
        (void)hipFuncSetAttribute((const void*)conv3d_igemm_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS_BYTES);
        attr = true;
    }
    if (one)
        hipLaunchKernelGGL(conv3d_igemm_kernel<true>, grid, dim3(256), S::LDS_BYTES, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(conv3d_igemm_kernel<false>, grid, dim3(256), S::LDS_BYTES, (hipStream_t)stream, p);
    MMVID_LAUNCH_CHECK("conv3d_ndhwc");
    return MMVID_OK;
}

extern "C" int mmvid_maxpool3d_ndhwc(const void* x, int N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw,
                                     int pt0, int pt1, int ph0, int ph1, int pw0, int pw1, void* out, int ldo, int c_off, void* stream) {
    MMVID_REQUIRE(x && out, "maxpool3d_ndhwc: null pointer");
    MMVID_REQUIRE(C % 8 == 0 && C > 0 && ldo % 8 == 0 && c_off % 8 == 0 && c_off >= 0 && c_off + C <= ldo,
                  "maxpool3d_ndhwc: C=%d, ldo=%d, c_off=%d must be multiples of 8 with the slice inside the output", C, ldo, c_off);
    MMVID_REQUIRE(N >= 0 && T > 0 && H > 0 && W > 0 && kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0 && pt0 >= 0 && pt1 >= 0 &&
                      ph0 >= 0 && ph1 >= 0 && pw0 >= 0 && pw1 >= 0 && pt0 < kt && ph0 < kh && pw0 < kw,
                  "maxpool3d_ndhwc: bad geometry");
    const int To = (T + pt0 + pt1 - kt) / st + 1, Ho = (H + ph0 + ph1 - kh) / sh + 1, Wo = (W + pw0 + pw1 - kw) / sw + 1;
    MMVID_REQUIRE(To > 0 && Ho > 0 && Wo > 0, "maxpool3d_ndhwc: empty output");
    const long total = (long)N * To * Ho * Wo * (C / 8);
    if (total == 0) return MMVID_OK;
    hipLaunchKernelGGL(maxpool3d_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, T, H, W, C, kt, kh, kw,
                       st, sh, sw, pt0, ph0, pw0, To, Ho, Wo, total, (bf16_t*)out, ldo, c_off);
    MMVID_LAUNCH_CHECK("maxpool3d_ndhwc");
    return MMVID_OK;
}

static int stem_pw0() { return 2; }  // TF-SAME on 224 columns, k 7, s 2: pad 5 = 2 front + 3 back

extern "C" int mmvid_i3d_preprocess(const float* videos, int n, int t, int h, int w, int video_length, void* out, void* stream) {
    MMVID_REQUIRE(videos && out, "i3d_preprocess: null pointer");
    MMVID_REQUIRE(n >= 0 && h > 0 && w > 0 && video_length > 0 && t > 0 && (t >= video_length || t >= 2),
                  "i3d_preprocess: t=%d frames cannot be extended to %d", t, video_length);
    const long total = (long)n * video_length * 224 * 112;
    MMVID_REQUIRE(total * 24 * 2 < (1l << 31), "i3d_preprocess: output of 2 GiB or more");
    if (total == 0) return MMVID_OK;
    hipLaunchKernelGGL(i3d_preprocess_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, videos, t, h, w, video_length, total,
                       stem_pw0(), (bf16_t*)out);
    MMVID_LAUNCH_CHECK("i3d_preprocess");
    return MMVID_OK;
}

extern "C" int mmvid_i3d_fold(const float* videos, int n, int t, void* out, void* stream) {
    MMVID_REQUIRE(videos && out && n >= 0 && t > 0, "i3d_fold: bad arguments");
    const long total = (long)n * t * 224 * 112;
    MMVID_REQUIRE(total * 24 * 2 < (1l << 31), "i3d_fold: output of 2 GiB or more");
    if (total == 0) return MMVID_OK;
    hipLaunchKernelGGL(i3d_fold_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, videos, total, stem_pw0(), (bf16_t*)out);
    MMVID_LAUNCH_CHECK("i3d_fold");
    return MMVID_OK;
}

extern "C" int mmvid_i3d_head(const void* x, int N, int To, int C, const float* w, const float* b, int ncls, float* out, void* stream) {
    MMVID_REQUIRE(x && w && b && out, "i3d_head: null pointer");
    MMVID_REQUIRE(To >= 2 && To - 1 <= HEAD_MAX_TP && C > 0 && C <= 1024 && ncls > 0,
                  "i3d_head: %d time steps (needs 2..%d) and C=%d (<= 1024)", To, HEAD_MAX_TP + 1, C);
    if (N == 0) return MMVID_OK;
    hipLaunchKernelGGL(i3d_head_kernel, dim3(N), dim3(256), (To - 1) * C * sizeof(float), (hipStream_t)stream, (const bf16_t*)x, To, C, w, b,
                       ncls, out);
    MMVID_LAUNCH_CHECK("i3d_head");
    return MMVID_OK;
}
