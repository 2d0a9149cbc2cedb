// Trainer telemetry (engine.FlatTrainer: telemetry_every): per-parameter statistics of the gradient, the weights and the update the
// optimiser just applied, read from the flat fp32 buffers and kept in a ring on the device.  include/mmvid_hip_ext.h states the rule;
// tests/telemetry_ref.py is its host replica, bit for bit.
//   per segment (one parameter): sum g^2 and max |g| over the finite g, the count of non-finite g, sum p^2, and sum d^2 with
//   d = ((lr / bc1) * m) / (sqrtf(v) / bc2s + eps), the update recomputed from the moments Adam left (0 where the guard skipped the step)
// Three launches, no host input, no atomics:
//   pass 1  256-thread blocks grid-stride over the list of chunks (MMVID_TELEMETRY_CHUNK = 4,096 elements of one segment); a block
//           reduces one chunk per trip and stores its partials.  Thread T holds elements 1024 r + 4 T + e (trip r, lane e) of the chunk:
//             q = (x0 x0 + x1 x1) + (x2 x2 + x3 x3) ;  a = (((0 + q0) + q1) + q2) + q3 ;  a wave: x[i] + x[i ^ 32], then ^ 16 ... ^ 1
//             (the halving tree: every lane ends with the same sum) ;  the block: (w0 + w1) + (w2 + w3)
//   pass 2  one block per segment: thread T adds chunk partials T, T + 256, ... in order, then the same wave and block tree; writes
//           the segment's record into the ring slot
//   finish  one block: the record's total (the pass-2 rule over the segments' g sums), the slot's header, count_dev += 1
// The order is a function of the segment's length and the chunk size alone.  A gated call (count % every != 0) returns from passes 1
// and 2 on a scalar branch before any load and only advances the counter.
// HBM-bound: 16 B read per parameter, each byte once (load_once: nontemporal), against the 28 B the Adam kernel moves.
// Pass 1 is bound by the bytes it keeps in flight, measured at BERT's 124.7 M elements ("Trainer telemetry"): a thread's
// four trips unrolled (16 float4 loads issued before the first use) at 8 waves per SIMD -- __launch_bounds__(256, 8): 64 VGPRs, 76 B of
// scratch per lane -- and 2,048 blocks take 0.356 ms (5.6 TB/s); the same loop at the 91 VGPRs it wants (5 waves) 0.414 ms with 1,024 or
// 2,048 blocks and 0.63 ms with 512; 6 or 7 waves 0.416 / 0.448; the trips not unrolled (70 VGPRs, 7 waves) 0.443, unrolled by two 0.449;
// the segment of a chunk carried from trip to trip in the place of the search 0.373 (no gain: the tables sit in the scalar cache).
// Table values are data: every address formed from a table is clipped to the buffers, every store index comes from the launch.
#include "../../include/mmvid_hip.h"
#include "../../include/mmvid_hip_ext.h"
#include "step_state.h"

// every product and sum of this file is the rounded fp32 operation it is written as: nothing is contracted into an fma
#pragma clang fp contract(off)

namespace {

constexpr long CHUNK = MMVID_TELEMETRY_CHUNK;
static_assert(CHUNK == 4 * 256 * 4, "a chunk is four trips of 256 threads x 4 elements");

struct Tables {
    const long* off;
    const long* len;
    const long* chunk0;
    int segments;
    long chunks;
};
// the segment's range as the kernels use it: the offset rounded down to a multiple of 4 and clipped to [0, n], the length to what is left
__device__ __forceinline__ void segment_range(const Tables& tb, int s, long n, long& off, long& len) {
    off = tb.off[s], len = tb.len[s];
    off = off < 0 ? 0 : (off > n ? n : off);
    off &= ~3L;
    len = len < 0 ? 0 : (len > n - off ? n - off : len);
}

struct Scalars {
    float lr, beta1, beta2, eps, bc1, bc2s;
    int step;
    const float* lr_dev;
    const float* step_dev;
    const int* skip;
};

__device__ __forceinline__ float quad(float a, float b, float c, float d) { return (a * a + b * b) + (c * c + d * d); }
__device__ __forceinline__ float update_of(float stepsz, float m, float v, float bc2s, float eps) {
    return (stepsz * m) / (sqrtf(v) / bc2s + eps);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Stats {
    float gsq, gmax, psq, dsq;
    int nonfinite, count;
};
// the block's tree: a wave's halving tree, then (w0 + w1) + (w2 + w3); the result is valid in thread 0.  Two barriers: the LDS is free
// again when it returns.
__device__ __forceinline__ Stats block_reduce(Stats a) {
    __shared__ float shf[4][4];
    __shared__ int shi[4][2];
    a.gsq = wave_sum(a.gsq), a.psq = wave_sum(a.psq), a.dsq = wave_sum(a.dsq), a.gmax = wave_max(a.gmax);
    a.nonfinite = wave_sum_i(a.nonfinite), a.count = wave_sum_i(a.count);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        shf[w][0] = a.gsq, shf[w][1] = a.gmax, shf[w][2] = a.psq, shf[w][3] = a.dsq;
        shi[w][0] = a.nonfinite, shi[w][1] = a.count;
    }
    __syncthreads();
    Stats r;
    r.gsq = (shf[0][0] + shf[1][0]) + (shf[2][0] + shf[3][0]);
    r.gmax = fmaxf(fmaxf(shf[0][1], shf[1][1]), fmaxf(shf[2][1], shf[3][1]));
    r.psq = (shf[0][2] + shf[1][2]) + (shf[2][2] + shf[3][2]);
    r.dsq = (shf[0][3] + shf[1][3]) + (shf[2][3] + shf[3][3]);
    r.nonfinite = (shi[0][0] + shi[1][0]) + (shi[2][0] + shi[3][0]);
    r.count = (shi[0][1] + shi[1][1]) + (shi[2][1] + shi[3][1]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool gated(int count, int every) { return (unsigned)count % (unsigned)every != 0; }
__device__ __forceinline__ long ring_slot(int count, int every, int slots) {
    return (long)(((unsigned)count / (unsigned)every) % (unsigned)slots);
}

__global__ __launch_bounds__(256, 8) void segment_chunks_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                             const float* __restrict__ m, const float* __restrict__ v, long n, Tables tb,
                                                             Scalars sc, LazyRows z, const int* __restrict__ count_dev, int every,
                                                             float* __restrict__ part_f, int* __restrict__ part_i) {
    if (gated(*count_dev, every)) return;  // a kernel argument's load, the same in every lane -- a scalar branch, before any other load
    const bool skipped = step_skipped(sc.skip);
    sc.lr = device_wins(sc.lr_dev, sc.lr);
    if (sc.step_dev) {
        const BiasCorrections bc = bias_corrections(sc.beta1, sc.beta2, *sc.step_dev);
        sc.bc1 = bc.bc1, sc.bc2s = bc.bc2_sqrt;
    }
    const float stepsz = sc.lr / sc.bc1;
    for (long c = blockIdx.x; c < tb.chunks; c += gridDim.x) {
        // the segment of chunk c: the last s with chunk0[s] <= c (a search over [0, segments): it ends and stays inside the table
        // whatever the table holds)
        int s = 0, hi = tb.segments - 1;
        while (s < hi) {
            const int mid = (s + hi + 1) >> 1;
            if (tb.chunk0[mid] <= c) s = mid;
            else hi = mid - 1;
        }
        long off, len;
        segment_range(tb, s, n, off, len);
        const long k = c - tb.chunk0[s];
        long cnt = 0, base = off;  // the chunk holds elements [base, base + cnt) of the flat buffers, inside [0, n)
        if (k >= 0 && k < (len + CHUNK - 1) / CHUNK) {
            base = off + k * CHUNK;
            cnt = len - k * CHUNK < CHUNK ? len - k * CHUNK : CHUNK;
        }
        Stats a = {0.f, 0.f, 0.f, 0.f, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long j = r * 1024 + (long)threadIdx.x * 4;
            if (j >= cnt) continue;
            const long i = base + j;
            float pe[4] = {0.f, 0.f, 0.f, 0.f}, ge[4] = {0.f, 0.f, 0.f, 0.f}, de[4] = {0.f, 0.f, 0.f, 0.f};
            if (j + 3 < cnt) {  // (base is a multiple of 4 and so is the lazy table's geometry: the four elements share a row)
                const bool lazy = lazy_skip(z, i);
                const f32x4 pp = load_once(p + i);
                pe[0] = pp.x, pe[1] = pp.y, pe[2] = pp.z, pe[3] = pp.w;
                if (!lazy) {
                    const f32x4 gg = load_once(g + i);
                    float gr[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool f = finite_bits(gr[e]);
                        ge[e] = f ? gr[e] : 0.f;
                        a.nonfinite += f ? 0 : 1;
                        a.gmax = fmaxf(a.gmax, fabsf(ge[e]));
                    }
                    a.count += 4;
                    if (!skipped) {
                        const f32x4 mm = load_once(m + i), vv = load_once(v + i);
                        de[0] = update_of(stepsz, mm.x, vv.x, sc.bc2s, sc.eps), de[1] = update_of(stepsz, mm.y, vv.y, sc.bc2s, sc.eps);
                        de[2] = update_of(stepsz, mm.z, vv.z, sc.bc2s, sc.eps), de[3] = update_of(stepsz, mm.w, vv.w, sc.bc2s, sc.eps);
                    }
                }
            } else {  // the last, partial group of the segment: element by element, what lies past the end stays +0
                for (int e = 0; e < 4 && j + e < cnt; ++e) {
                    pe[e] = p[i + e];
                    if (lazy_skip(z, i + e)) continue;
                    const float x = g[i + e];
                    const bool f = finite_bits(x);
                    ge[e] = f ? x : 0.f;
                    a.nonfinite += f ? 0 : 1;
                    a.gmax = fmaxf(a.gmax, fabsf(ge[e]));
                    a.count += 1;
                    if (!skipped) de[e] = update_of(stepsz, m[i + e], v[i + e], sc.bc2s, sc.eps);
                }
            }
            a.gsq = a.gsq + quad(ge[0], ge[1], ge[2], ge[3]);
            a.psq = a.psq + quad(pe[0], pe[1], pe[2], pe[3]);
            a.dsq = a.dsq + quad(de[0], de[1], de[2], de[3]);
        }
        const Stats t = block_reduce(a);
        if (threadIdx.x == 0) {
            part_f[c * 4 + 0] = t.gsq, part_f[c * 4 + 1] = t.gmax, part_f[c * 4 + 2] = t.psq, part_f[c * 4 + 3] = t.dsq;
            part_i[c * 2 + 0] = t.nonfinite, part_i[c * 2 + 1] = t.count;
        }
    }
}

__global__ __launch_bounds__(256) void segment_sum_kernel(long n, Tables tb, const int* __restrict__ count_dev, int every, int slots,
                                                          const float* __restrict__ part_f, const int* __restrict__ part_i,
                                                          float* __restrict__ ring_f, int* __restrict__ ring_i) {
    const int count = *count_dev;
    if (gated(count, every)) return;
    const int s = blockIdx.x;  // < segments: the grid
    long off, len;
    segment_range(tb, s, n, off, len);
    long c0 = tb.chunk0[s];
    c0 = c0 < 0 ? 0 : (c0 > tb.chunks ? tb.chunks : c0);
    long nc = (len + CHUNK - 1) / CHUNK;
    if (nc > tb.chunks - c0) nc = tb.chunks - c0;
    Stats a = {0.f, 0.f, 0.f, 0.f, 0, 0};
    for (long i = threadIdx.x; i < nc; i += 256) {
        const long c = c0 + i;
        a.gsq = a.gsq + part_f[c * 4 + 0], a.gmax = fmaxf(a.gmax, part_f[c * 4 + 1]);
        a.psq = a.psq + part_f[c * 4 + 2], a.dsq = a.dsq + part_f[c * 4 + 3];
        a.nonfinite += part_i[c * 2 + 0], a.count += part_i[c * 2 + 1];
    }
    const Stats t = block_reduce(a);
    if (threadIdx.x == 0) {
        const long at = ring_slot(count, every, slots) * tb.segments + s;
        ring_f[at * 4 + 0] = t.gsq, ring_f[at * 4 + 1] = t.gmax, ring_f[at * 4 + 2] = t.psq, ring_f[at * 4 + 3] = t.dsq;
        ring_i[at * 2 + 0] = t.nonfinite, ring_i[at * 2 + 1] = t.count;
    }
}

__global__ __launch_bounds__(256) void segment_finish_kernel(int segments, Scalars sc, int* __restrict__ count_dev, int every, int slots,
                                                             const float* __restrict__ ring_f, int* __restrict__ head_i,
                                                             float* __restrict__ head_f) {
    const int count = *count_dev;
    if (!gated(count, every)) {  // (the same in every thread: all of them reach the barriers of block_reduce)
        const long slot = ring_slot(count, every, slots);
        Stats a = {0.f, 0.f, 0.f, 0.f, 0, 0};
        for (int s = threadIdx.x; s < segments; s += 256) a.gsq = a.gsq + ring_f[(slot * segments + s) * 4];
        const Stats t = block_reduce(a);
        if (threadIdx.x == 0) {
            head_i[slot * 4 + 0] = count;
            head_i[slot * 4 + 1] = sc.step_dev ? (int)*sc.step_dev : sc.step;
            head_i[slot * 4 + 2] = step_skipped(sc.skip) ? 1 : 0;
            head_i[slot * 4 + 3] = 1;
            head_f[slot * 2 + 0] = device_wins(sc.lr_dev, sc.lr);
            head_f[slot * 2 + 1] = t.gsq;
        }
    }
    __syncthreads();  // every thread holds `count` (its branch above used it) before thread 0 overwrites it
    if (threadIdx.x == 0) *count_dev = (int)((unsigned)count + 1u);
}

}  // namespace

extern "C" int mmvid_segment_stats(const float* g, const float* p, const float* m, const float* v, int64_t n, const int64_t* seg_off,
                                   const int64_t* seg_len, const int64_t* seg_chunk0, int32_t segments, int64_t chunks, float lr,
                                   const float* lr_dev, float beta1, float beta2, float eps, int step, const float* step_dev,
                                   const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, const int32_t* skip_dev,
                                   int32_t every, int32_t slots, int32_t* count_dev, float* partials_f, int32_t* partials_i,
                                   float* ring_f, int32_t* ring_i, int32_t* head_i, float* head_f, void* stream) {
    MMVID_REQUIRE(g && p && m && v, "segment_stats: g, p, m and v must not be NULL");
    MMVID_REQUIRE(seg_off && seg_len && seg_chunk0, "segment_stats: the segment tables must not be NULL");
    MMVID_REQUIRE(count_dev && partials_f && partials_i && ring_f && ring_i && head_i && head_f,
                  "segment_stats: count_dev, the partials, the ring and its headers must not be NULL");
    MMVID_REQUIRE((((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
                  "segment_stats: g, p, m and v must be 16-byte aligned");
    MMVID_REQUIRE((((uintptr_t)seg_off | (uintptr_t)seg_len | (uintptr_t)seg_chunk0) & 7) == 0,
                  "segment_stats: the segment tables must be 8-byte aligned");
    MMVID_REQUIRE((((uintptr_t)lr_dev | (uintptr_t)step_dev | (uintptr_t)skip_dev | (uintptr_t)count_dev | (uintptr_t)partials_f |
                    (uintptr_t)partials_i | (uintptr_t)ring_f | (uintptr_t)ring_i | (uintptr_t)head_i | (uintptr_t)head_f) & 3) == 0,
                  "segment_stats: lr_dev, step_dev, skip_dev, count_dev, the partials, the ring and its headers must be 4-byte aligned");
    MMVID_REQUIRE(n >= 0 && n <= (int64_t)1 << 60, "segment_stats: n=%lld is negative (or beyond 2^60)", (long long)n);
    MMVID_REQUIRE(segments >= 1 && segments <= MMVID_TELEMETRY_MAX_SEGMENTS, "segment_stats: segments=%d is outside [1, %d]", segments,
                  MMVID_TELEMETRY_MAX_SEGMENTS);
    MMVID_REQUIRE(chunks >= segments && chunks <= n / CHUNK + segments,
                  "segment_stats: chunks=%lld is outside [segments, n / %ld + segments] = [%d, %lld]", (long long)chunks, CHUNK, segments,
                  (long long)(n / CHUNK + segments));
    MMVID_REQUIRE(every >= 1 && slots >= 1, "segment_stats: every=%d and slots=%d must be >= 1", every, slots);
    MMVID_REQUIRE(step >= 1 || step_dev, "segment_stats: step=%d must be >= 1 where no device step count is given", step);
    MMVID_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "segment_stats: beta1=%g or beta2=%g is outside [0, 1)",
                  (double)beta1, (double)beta2);  // (false for NaN)
    LazyRows z;
    if (int rc = make_lazy(z, "segment_stats", row_flags, table_lo, table_rows, rowlen, n)) return rc;
    if (n == 0) return MMVID_OK;
    Tables tb;
    tb.off = (const long*)seg_off, tb.len = (const long*)seg_len, tb.chunk0 = (const long*)seg_chunk0, tb.segments = segments, tb.chunks = chunks;
    Scalars sc;
    sc.lr = lr, sc.beta1 = beta1, sc.beta2 = beta2, sc.eps = eps, sc.step = step >= 1 ? step : 1;
    const BiasCorrections bc = bias_corrections(beta1, beta2, (float)sc.step);
    sc.bc1 = bc.bc1, sc.bc2s = bc.bc2_sqrt;
    sc.lr_dev = lr_dev, sc.step_dev = step_dev, sc.skip = (const int*)skip_dev;
    const unsigned blocks = (unsigned)(chunks < 2048 ? chunks : 2048);  // eight blocks per CU, all resident: see the head of this file
    hipLaunchKernelGGL(segment_chunks_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, p, m, v, (long)n, tb, sc, z,
                       (const int*)count_dev, every, partials_f, (int*)partials_i);
    hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)segments), dim3(256), 0, (hipStream_t)stream, (long)n, tb, (const int*)count_dev,
                       every, slots, (const float*)partials_f, (const int*)partials_i, ring_f, (int*)ring_i);
    hipLaunchKernelGGL(segment_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, segments, sc, (int*)count_dev, every, slots,
                       (const float*)ring_f, (int*)head_i, head_f);
    MMVID_LAUNCH_CHECK("segment_stats");
    return MMVID_OK;
}
