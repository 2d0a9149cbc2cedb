// Seeded sampling: the samplers' race variates as a pure function of (video seed, purpose, substream, draw number, index), made on
// the device into the tensors the draw kernels (sample.hip) already read.  include/mmvid_hip_ext.h states the function and the
// layout; tests/variates_ref.py is its host replica.
//
// A video's rows_per_video * n variates of one draw lie contiguous in `out` and in index order (row r, column c of the video is index
// r * n + c), so a launch is `draws * videos` independent segments of L = rows_per_video * n floats, segment (k, v) at out + (k * videos
// + v) * L, and inside a segment float i is variate i: a row that starts at i % 4 != 0 simply starts inside a Philox block.  One thread
// makes one Philox block = floats 4j .. 4j+3 of its segment: 16 B per lane, consecutive lanes consecutive blocks, one 1 KiB store per
// wave when the segments are 16-byte aligned (L % 4 == 0, as every call of the samplers is: V and TS are multiples of 4) and four
// dword stores otherwise.  Per 16 B stored a thread spends the 20 32x32->64 multiplies of the ten rounds (quarter rate), which is
// about the HBM write rate of the chip: the kernel is a few microseconds against a tower pass.
#include "../../include/mmvid_hip_ext.h"
#include "common.h"
#include "philox.h"

namespace {

template <bool VEC, int KIND>
__global__ __launch_bounds__(256) void variates_fill_kernel(const long long* __restrict__ seeds, const int* __restrict__ substream,
                                                            long videos, long L, uint32_t purpose, const int* __restrict__ draw_dev,
                                                            long long draw_first, long segs, float* __restrict__ out) {
    const unsigned long long nblk = ((unsigned long long)L + 3ull) >> 2;  // Philox blocks per segment: <= 2^32
    const long long d0 = draw_first + (draw_dev ? (long long)draw_dev[0] : 0ll);
    for (long s = blockIdx.y; s < segs; s += gridDim.y) {
        const long k = s / videos, v = s - k * videos;  // (uniform over the block: scalar)
        const unsigned long long seed = (unsigned long long)seeds[v];
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), sub = substream ? (uint32_t)substream[v] : 0u;
        const uint32_t draw = (uint32_t)(d0 + k);
        float* __restrict__ seg = out + s * L;
        for (unsigned long long j = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; j < nblk; j += (unsigned long long)gridDim.x * 256ull) {
            const U4 r = philox((uint32_t)j, purpose, sub, draw, k0, k1);
            const float f0 = KIND ? exp1(r.x) : u01(r.x), f1 = KIND ? exp1(r.y) : u01(r.y), f2 = KIND ? exp1(r.z) : u01(r.z),
                        f3 = KIND ? exp1(r.w) : u01(r.w);
            const unsigned long long i = j << 2;  // < L <= 2^34
            if (VEC) {  // L % 4 == 0: the block is whole, and 16-byte aligned
                *reinterpret_cast<f32x4*>(seg + i) = f32x4{f0, f1, f2, f3};
            } else {
                seg[i] = f0;
                if (i + 1 < (unsigned long long)L) seg[i + 1] = f1;
                if (i + 2 < (unsigned long long)L) seg[i + 2] = f2;
                if (i + 3 < (unsigned long long)L) seg[i + 3] = f3;
            }
        }
    }
}

}  // namespace

extern "C" int mmvid_variates_fill(const int64_t* seeds, const int32_t* substream, int64_t videos, int64_t rows_per_video, int64_t n,
                                   int purpose, int kind, const int32_t* draw_dev, int64_t draw_first, int64_t draws, float* out,
                                   void* stream) {
    MMVID_REQUIRE(seeds && out, "variates_fill: seeds and out must not be NULL");
    MMVID_REQUIRE(videos >= 0 && rows_per_video >= 0 && n >= 0 && draws >= 0, "variates_fill: negative size (videos=%ld rows_per_video=%ld n=%ld draws=%ld)",
                  (long)videos, (long)rows_per_video, (long)n, (long)draws);
    MMVID_REQUIRE(purpose >= 1 && purpose <= 3, "variates_fill: purpose=%d is outside 1..3 (token race, token noise, keep race)", purpose);
    MMVID_REQUIRE(kind == 0 || kind == 1, "variates_fill: kind=%d is outside 0..1 (uniform, Exp(1))", kind);
    const int64_t LMAX = (int64_t)1 << 34;
    MMVID_REQUIRE(rows_per_video == 0 || n <= LMAX / rows_per_video, "variates_fill: rows_per_video * n = %ld * %ld exceeds 2^34 (the block index must fit a 32-bit counter word)",
                  (long)rows_per_video, (long)n);
    if (draw_dev) {
        MMVID_REQUIRE(draws == 1, "variates_fill: a device-side draw number makes one draw, got draws=%ld", (long)draws);
        MMVID_REQUIRE(draw_first > -((int64_t)1 << 32) && draw_first < ((int64_t)1 << 32), "variates_fill: draw_first=%ld is outside (-2^32, 2^32)", (long)draw_first);
    } else {
        MMVID_REQUIRE(draw_first >= 0 && draws <= ((int64_t)1 << 32) && draw_first <= ((int64_t)1 << 32) - draws,
                      "variates_fill: draw numbers %ld .. %ld + %ld are outside [0, 2^32)", (long)draw_first, (long)draw_first, (long)draws);
    }
    const int64_t L = rows_per_video * n;
    if (videos == 0 || L == 0 || draws == 0) return MMVID_OK;
    MMVID_REQUIRE(draws <= INT64_MAX / videos && draws * videos <= INT64_MAX / L, "variates_fill: draws * videos * rows_per_video * n overflows 63 bits");
    const int64_t segs = draws * videos, nblk = (L + 3) >> 2, bx = (nblk + 255) / 256;
    // at most 2^10 x 2^13 blocks of 256 threads (a launch holds fewer than 2^32 threads); the kernel strides over the rest
    const dim3 grid((unsigned)(bx < 1024 ? bx : 1024), (unsigned)(segs < 8192 ? segs : 8192));
    const bool vec = L % 4 == 0 && ((uintptr_t)out & 15u) == 0;
#define MMVID_VARIATES_LAUNCH(VEC, KIND)                                                                                                   \
    hipLaunchKernelGGL((variates_fill_kernel<VEC, KIND>), grid, dim3(256), 0, (hipStream_t)stream, (const long long*)seeds, (const int*)substream, \
                       (long)videos, (long)L, (uint32_t)purpose, (const int*)draw_dev, (long long)draw_first, (long)segs, out)
    if (vec) {
        if (kind) MMVID_VARIATES_LAUNCH(true, 1);
        else MMVID_VARIATES_LAUNCH(true, 0);
    } else {
        if (kind) MMVID_VARIATES_LAUNCH(false, 1);
        else MMVID_VARIATES_LAUNCH(false, 0);
    }
#undef MMVID_VARIATES_LAUNCH
    MMVID_LAUNCH_CHECK("variates_fill");
    return MMVID_OK;
}
